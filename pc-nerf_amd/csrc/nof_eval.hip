// Eval-mode NOF query: positional encoding + the full 9-Linear network + sigmoid, fused in one kernel with
// every activation held in registers (nof/networks/models.py:27-41 Embedding, :183-203 NOF_coarse.forward;
// render.py:18-25 chunk loop).  BatchNorm1d in eval mode is an affine map per feature, folded into the
// Linear that produces it when the network image is packed (pcnerf_nof_pack_eval).
//
// MFMA mapping (v_mfma_f32_32x32x2_f32, exact fp32 fmaf chain).  One wave owns a tile of 32 samples and
// computes every layer transposed, out^T[neuron][sample] = W[neuron][:] . act^T[:][sample]:
//   A operand (lane l) = W[32*ob + (l&31)][feature(t, l>>5)]      -- packed weights, 1 VGPR per k-step
//   B operand (lane l) = act[feature(t, l>>5)][sample l&31]      -- register-resident activations
//   D (block ob, reg r, lane l) = out[32*ob + (r&3) + 8*(r>>2) + 4*(l>>5)][sample l&31]
// so accumulator register R = 16*ob + r of a layer IS the B operand of k-step t = R of the next layer
// (feature map FEAT_H below): the whole chain runs without LDS or lane shuffles.  The encoding feeds layer 1
// (and the skip half of layer 5) with feature(t, h) = 2t + h.
#include <algorithm>
#include <type_traits>

#include "common.h"
#include "pcnerf_internal.h"
#include "prof.h"

namespace pcn {

// ---------------------------------------------------------------------------------- eval network image
// [L1e][L2h][L3h][L4h][L5e][L5h][L6h][L7h][L8h][bias 8x256][w_out 256][b_out 4]
// e-part: KG_E = 8 groups of 4 k-steps (64 features, the 64th is zero padding); h-part: KG_H = 32 groups.
// Within a part: [kg][ob(8)][lane(64)][q(4)], value = W'[32*ob + (lane&31)][feature(4*kg+q, lane>>5)].
constexpr int KG_E = 8, KG_H = 32;
constexpr size_t SZ_E = (size_t)KG_E * 8 * 64 * 4;  // 16384
constexpr size_t SZ_H = (size_t)KG_H * 8 * 64 * 4;  // 65536
__host__ __device__ constexpr size_t off_w(int layer, bool epart) {
  // layer 0..7
  return layer == 0 ? 0
       : layer <= 3 ? SZ_E + (size_t)(layer - 1) * SZ_H
       : layer == 4 ? (epart ? SZ_E + 3 * SZ_H : 2 * SZ_E + 3 * SZ_H)
                    : 2 * SZ_E + (size_t)(layer - 1) * SZ_H;
}
constexpr size_t OFF_BIAS = 2 * SZ_E + 7 * SZ_H;
constexpr size_t OFF_WOUT = OFF_BIAS + 8 * 256;
constexpr size_t OFF_BOUT = OFF_WOUT + 256;
constexpr size_t EVAL_F32_FLOATS = OFF_BOUT + 4;   // the fp32 image (k_nof_eval)
// split-fp16 image (k_nof_eval_h3), appended: [sw: 8 int32 exponents, 16-float aligned][60 k-steps][16 neuron
// blocks][part 2][lane 64] f16x8 (see k_nof_eval_h3)
// [lane 64] f16x8 -- the eval network's 120 k-steps of 16 features (layer 0: 4, layers 1-3, 5-7: 16, layer 4: 4 + 16)
constexpr int EH3_KSTEPS = 60;
constexpr size_t EH_VECS = (size_t)EH3_KSTEPS * 16 * 2 * 64;
constexpr size_t OFF_EH_SW = EVAL_F32_FLOATS;
constexpr size_t OFF_EH = OFF_EH_SW + 16;
constexpr size_t EVAL_FLOATS = OFF_EH + EH_VECS * 4;
static_assert(EVAL_F32_FLOATS % 4 == 0, "f16x8 alignment of the split image");

__device__ __forceinline__ int feat_h(int t, int h) {  // accumulator register -> neuron
  return 32 * (t >> 4) + (t & 3) + 8 * ((t & 15) >> 2) + 4 * h;
}

// one thread per packed float of the weight parts
__global__ void k_pack_eval_weights(NofParamsDev P, float* __restrict__ out) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= OFF_BIAS) return;
  int layer;
  bool epart;
  size_t base;
  if (idx < SZ_E) { layer = 0; epart = true; base = 0; }
  else if (idx < SZ_E + 3 * SZ_H) { layer = 1 + (int)((idx - SZ_E) / SZ_H); epart = false; base = off_w(layer, false); }
  else if (idx < 2 * SZ_E + 3 * SZ_H) { layer = 4; epart = true; base = off_w(4, true); }
  else if (idx < 2 * SZ_E + 4 * SZ_H) { layer = 4; epart = false; base = off_w(4, false); }
  else { layer = 5 + (int)((idx - (2 * SZ_E + 4 * SZ_H)) / SZ_H); epart = false; base = off_w(layer, false); }
  const size_t j = idx - base;
  const int q = (int)(j & 3), lane = (int)((j >> 2) & 63), ob = (int)((j >> 8) & 7), kg = (int)(j >> 11);
  const int t = 4 * kg + q, h = lane >> 5, n = 32 * ob + (lane & 31);
  const int in_f = layer == 0 ? 63 : layer == 4 ? 319 : 256;
  int col;
  if (epart) {
    const int f = 2 * t + h;
    col = f < 63 ? f : -1;
  } else {
    col = (layer == 4 ? 63 : 0) + feat_h(t, h);
  }
  // BatchNorm eval: alpha = gamma / sqrt(rv + eps) (ATen batch_norm_cpu_transform_input: invstd * weight)
  const float alpha = (1.0f / sqrtf(P.bn_rv[layer][n] + P.eps)) * P.bn_w[layer][n];
  out[idx] = col < 0 ? 0.0f : alpha * P.lin_w[layer][(size_t)n * in_f + col];
}

// RAW (the train query's image): the Linear biases as they are (its activation-store writes add them to W x)
template <bool RAW>
__global__ void k_pack_eval_vectors(NofParamsDev P, float* __restrict__ out) {
  const int n = threadIdx.x;  // 256 threads
  for (int layer = 0; layer < 8; ++layer) {
    if (RAW) {
      out[OFF_BIAS + layer * 256 + n] = P.lin_b[layer][n];
      continue;
    }
    const float alpha = (1.0f / sqrtf(P.bn_rv[layer][n] + P.eps)) * P.bn_w[layer][n];
    const float beta = P.bn_b[layer][n] - P.bn_rm[layer][n] * alpha;
    out[OFF_BIAS + layer * 256 + n] = alpha * P.lin_b[layer][n] + beta;
  }
  out[OFF_WOUT + n] = P.out_w[n];
  if (n == 0) {
    out[OFF_BOUT] = P.out_b[0];
    out[OFF_BOUT + 1] = out[OFF_BOUT + 2] = out[OFF_BOUT + 3] = 0.0f;
  }
}

// ---------------------------------------------------------------------------------- fused query kernel

template <int KG, int NX>
__device__ __forceinline__ void gemm_t(f32x16 (&acc)[8], const float (&x)[NX], const float* __restrict__ wp,
                                       int lane) {
  static_assert(NX == 4 * KG, "operand count");
  const f32x4* __restrict__ w4 = reinterpret_cast<const f32x4*>(wp) + lane;
  f32x4 wa[8];
#pragma unroll
  for (int ob = 0; ob < 8; ++ob) wa[ob] = w4[ob * 64];
#pragma unroll
  for (int kg = 0; kg < KG; ++kg) {
    f32x4 wb[8];
    if (kg + 1 < KG) {
#pragma unroll
      for (int ob = 0; ob < 8; ++ob) wb[ob] = w4[((kg + 1) * 8 + ob) * 64];
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
#pragma unroll
      for (int ob = 0; ob < 8; ++ob)
        acc[ob] = __builtin_amdgcn_mfma_f32_32x32x2f32(wa[ob][q], x[4 * kg + q], acc[ob], 0, 0, 0);
    }
    if (kg + 1 < KG) {
#pragma unroll
      for (int ob = 0; ob < 8; ++ob) wa[ob] = wb[ob];
    }
  }
}

__device__ __forceinline__ void init_bias_t(f32x16 (&acc)[8], const float* __restrict__ b, int h) {
#pragma unroll
  for (int ob = 0; ob < 8; ++ob) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(b + 32 * ob + 8 * g + 4 * h);
      acc[ob][4 * g + 0] = v[0];
      acc[ob][4 * g + 1] = v[1];
      acc[ob][4 * g + 2] = v[2];
      acc[ob][4 * g + 3] = v[3];
    }
  }
}

// ein != NULL: the (total, 63) embedding is read from memory instead (NOF.forward on embedded input).
__global__ __launch_bounds__(256) void k_nof_eval(const float* __restrict__ rays, int stride,
                                                  const float* __restrict__ z, int64_t total, int S,
                                                  const float* __restrict__ ein, const float* __restrict__ W,
                                                  float* __restrict__ p_out) {
  const int lane = threadIdx.x & 63, h = lane >> 5;
  const int64_t tile = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t g = tile * 32 + (lane & 31);
  const int64_t gc = g < total ? g : total - 1;
  float e[32];
  if (ein) {
    load_embedding<0>(ein + gc * 63, h, e);
  } else {
    const float* r = rays + ray_of(gc, S) * stride;
    float p[3];
    sample_point(r, z[gc], p);
    encode_half(p, h, e);
  }

  // the 8 layers' biases in LDS (one 8 KiB copy per block): each layer's accumulator initialisation is then an
  // LDS read instead of 32 global loads whose latency stalled the layer's first MFMA
  __shared__ __attribute__((aligned(16))) float sbias[8 * 256];
  for (int i = threadIdx.x; i < 8 * 256 / 4; i += blockDim.x)
    reinterpret_cast<f32x4*>(sbias)[i] = reinterpret_cast<const f32x4*>(W + OFF_BIAS)[i];
  __syncthreads();
  f32x16 acc[8];
  float act[128];
#pragma unroll 1
  for (int L = 0; L < 8; ++L) {
    init_bias_t(acc, sbias + 256 * L, h);
    if (L == 0 || L == 4) gemm_t<KG_E>(acc, e, W + off_w(L, true), lane);
    if (L != 0) gemm_t<KG_H>(acc, act, W + off_w(L, false), lane);
#pragma unroll
    for (int R = 0; R < 128; ++R) act[R] = acc[R >> 4][R & 15];
  }
  // occ_out: Linear(256, 1) + Sigmoid; each lane holds half the features of its sample
  float part = 0.0f;
#pragma unroll
  for (int ob = 0; ob < 8; ++ob) {
#pragma unroll
    for (int gq = 0; gq < 4; ++gq) {
      const f32x4 wv = *reinterpret_cast<const f32x4*>(W + OFF_WOUT + 32 * ob + 8 * gq + 4 * h);
#pragma unroll
      for (int q = 0; q < 4; ++q) part = fmaf(wv[q], act[16 * ob + 4 * gq + q], part);
    }
  }
  const float logit = part + __shfl_xor(part, 32, 64) + W[OFF_BOUT];
  if (lane < 32 && g < total) p_out[g] = sigmoid_ref(logit);
}

// ---------------------------------------------------------------------------------- split-fp16 eval query
// k_nof_eval's fused network with every fp32 product rebuilt from fp16 parts on v_mfma_f32_32x32x16_f16 (the
// split train math, DESIGN "The split train math"): v = hi + mid (22 significant bits), W x = Wh xh + Wh xm + Wm xh,
// exact products, fp32 accumulation.  Scales are powers of two undone in each layer's epilogue: per layer for the
// BatchNorm-folded weights (max |W'| 2^sw in [2^14, 2^15)), per SAMPLE for the activations (max over the sample's
// features, so a sample's result never depends on the other samples of its tile).
// One wave owns 32 samples (as k_nof_eval); a block of 4 waves (one per SIMD: 128 accumulator + 128 activation
// registers per lane) shares the weight stream: each k-step's 16 KiB slice (8 out-blocks x hi/mid) is loaded two
// k-steps ahead by all 256 threads and published in one of two LDS slots, one barrier per k-step.
// Operand maps: A (lane l) = W'[32 ob + (l&31)][col(s, l>>5, j)], B (lane l) = x[col(s, l>>5, j)][sample l&31],
// j = 0..7, with col(s, h, j) = 2 (8 s + j) + h for the encoding (encode_half's e[8 s + j]) and
// 16 s + 8 (j>>2) + 4 h + (j&3) for the 256 hidden features -- exactly accumulator registers 8 (s&1) + j of
// block s>>1 of the previous layer, so each layer's B operands are its predecessor's accumulators split in place.

// per-layer weight scale exponents of the BatchNorm-folded weights (RAW: of the raw weights, for the train-mode
// query), stored in the image as int32
template <bool RAW>
__global__ __launch_bounds__(1024) void k_eval_wscale(NofParamsDev P, float* __restrict__ out) {
  const int L = blockIdx.x;
  const float m = block_layer_absmax<1024>(P.lin_w[L], 256, L == 0 ? 63 : L == 4 ? 319 : 256, [&](int n) {
    return RAW ? 1.0f : (1.0f / sqrtf(P.bn_rv[L][n] + P.eps)) * P.bn_w[L][n];
  });
  if (threadIdx.x == 0) reinterpret_cast<int*>(out + OFF_EH_SW)[L] = m > 0.0f && m == m && m < 3.0e38f ? 14 - ilogbf(m) : 0;
}

typedef _Float16 eh_f16x8 __attribute__((ext_vector_type(8)));

// the per-sample scale exponent for a max |x| (0 for zero / non-finite maxima), clamped so that every unscale
// factor stays a normal float
__device__ __forceinline__ int eh_scale(float m) {
  int e = (m > 0.0f && m < 3.0e38f) ? 14 - ilogbf(m) : 0;
  return e > 64 ? 64 : e < -64 ? -64 : e;
}

// 8 values -> hi / mid fp16 parts, the low part from ONE mixed-precision fma per value, mid = f16(v - f32(hi))
// (v_fma_mix{lo,hi}_f16, the f16 operand selected by op_sel): v - hi is exact in fp32 (hi is v rounded to 11 bits),
// so this is the same single rounding as converting the fp32 difference -- bit for bit (scripts/micro/split_mix.hip
// checks it on the GPU over 67M values) -- in 3 instructions per pair instead of 5 (query time -0.6 %)
__device__ __forceinline__ void eh_split8(const float (&v)[8], eh_f16x8& hi, eh_f16x8& mid) {
  typedef _Float16 eh_f16x2 __attribute__((ext_vector_type(2)));
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    eh_f16x2 hp;
    hp[0] = (_Float16)v[2 * p];
    hp[1] = (_Float16)v[2 * p + 1];
    const unsigned hb = __builtin_bit_cast(unsigned, hp);
    unsigned mb;
    asm("v_fma_mixlo_f16 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(mb) : "v"(hb), "v"(v[2 * p]));
    asm("v_fma_mixhi_f16 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "+v"(mb) : "v"(hb), "v"(v[2 * p + 1]));
    const eh_f16x2 mp = __builtin_bit_cast(eh_f16x2, mb);
    hi[2 * p] = hp[0];
    hi[2 * p + 1] = hp[1];
    mid[2 * p] = mp[0];
    mid[2 * p + 1] = mp[1];
  }
}

// ---- k_nof_eval_h3: the split network (every fp32 product as hi*hi + hi*mid + mid*hi of fp16 parts, fp32
// accumulation), fused over all 9 layers for a block of 16 SB samples with the work split over NEURONS: wave w of NW
// owns J = 16 / NW neuron blocks (neurons 16 J w .. 16 J (w + 1) - 1) of every layer for all the block's samples, so
// each wave streams only its own neurons' weights from L2 (an R3-slot register ring, R3 - 1 k-steps of prefetch, no
// barrier) and each A operand feeds SB sample blocks.  Two geometries, two waves per SIMD on a CU either way:
// <NW 4, SB 3> (two workgroups of 48 samples per CU, each streaming the whole image: the eval query and the
// store-writing train query) and <NW 8, SB 6, 7 or 8> (one workgroup of 96, 112 or 128 samples, one pass over the image:
// the store-less train query, 8 blocks by default -- EH3_TRAIN_FORM below);
// every accumulator sees the same products in the same order in all of them (the formulas below are for NW = 4: J = 4);
// the layer outputs go through LDS as the next layer's split B operands ([k-step][sample block][part][lane],
// 16 KiB per sample block), two barriers per layer.  The encoding lives in LDS as layer 0's split B operands; layer 4 re-splits it
// (hi + mid is exact in fp32) at the per-sample scale it shares with h3.
// On v_mfma_f32_16x16x32_f16: 4 neuron blocks x EH3_SB sample blocks of 16, k-steps of 32 features.  Against the same
// block on 32x32x16 (2 x 3 blocks of 32, k-steps of 16; round 3's k_nof_eval_h2, in git history) it is 4-7 %
// faster in the train query and 1-2 % in the eval query (profiles/r03l_variants_eval_*.json): the kernel runs
// power-limited (DESIGN (f)), and at the same issue rate the smaller shape draws less power per FLOP
// (scripts/micro/mfma_f16_shape.hip with LDS B operands: 1.79 PF at 1.80 GHz vs 1.63 PF at 1.61 GHz).
// Operand maps (16x16x32: lane l = column l & 15, k-group g = l >> 4 holding k = 8g .. 8g + 7; D reg r of lane l =
// row 4g + r, column l & 15):
//   accumulator acc[j][sb] reg r, lane l = neuron 64w + 16j + 4g + r of sample 16sb + (l & 15);
//   (NW = 8: neuron 32w + 16j + 4g + r, and act[w] below)
//   a layer's output in LDS: act[2w + jp][sb][part][l] = (acc[2jp][sb][0..3], acc[2jp + 1][sb][0..3]) of lane l, so
//   hidden k-step s, k-group g, element e is input neuron 32s + 16(e >> 2) + 4g + (e & 3) (the image's column map);
//   the encoding: eb[s][sb][part][l] element e = feature 32s + 8g + e (63: zero padding).
// Image: [60 k-steps][16 neuron blocks][part 2][lane 64] f16x8 (layer 0: 2 k-steps, 1-3 / 5-7: 8, layer 4: 2 + 8),
// 1.97 MB.
__host__ __device__ constexpr int eh3_start(int L) { return L == 0 ? 0 : L <= 4 ? 2 + 8 * (L - 1) : 4 + 8 * (L - 1); }
static_assert(eh3_start(7) + 8 == EH3_KSTEPS, "k-steps of the image");

template <bool RAW>
__global__ void k_pack_eval_h3(NofParamsDev P, float* __restrict__ out) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= EH_VECS) return;
  const int lane = (int)(idx & 63), part = (int)((idx >> 6) & 1), nb = (int)((idx >> 7) & 15);
  const int gk = (int)(idx >> 11);
  int L = 0;
  while (L < 7 && gk >= eh3_start(L + 1)) ++L;
  const int s0 = gk - eh3_start(L);
  const bool epart = L == 0 || (L == 4 && s0 < 2);
  const int s = L == 4 && !epart ? s0 - 2 : s0;
  const int n = 16 * nb + (lane & 15), g = lane >> 4;
  const int in_f = L == 0 ? 63 : L == 4 ? 319 : 256;
  const float alpha = RAW ? 1.0f : (1.0f / sqrtf(P.bn_rv[L][n] + P.eps)) * P.bn_w[L][n];
  const float sc = ldexpf(1.0f, reinterpret_cast<const int*>(out + OFF_EH_SW)[L]);
  eh_f16x8 v;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    int col;
    if (epart) {
      const int f = 32 * s + 8 * g + e;
      col = f < 63 ? f : -1;
    } else {
      col = (L == 4 ? 63 : 0) + 32 * s + 16 * (e >> 2) + 4 * g + (e & 3);
    }
    const float w = col < 0 ? 0.0f : (alpha * P.lin_w[L][(size_t)n * in_f + col]) * sc;
    const _Float16 hi = (_Float16)w;
    v[e] = part == 0 ? hi : (_Float16)(w - (float)hi);
  }
  reinterpret_cast<eh_f16x8*>(out + OFF_EH)[idx] = v;
}

// 16-sample blocks per workgroup, and workgroups per CU.  Three blocks (77.5 KiB of LDS in the train form) let TWO
// workgroups share a CU (two waves per SIMD, <= 256 registers each, no spills), so one workgroup's layer transitions
// (barriers, epilogue, split) and prologue run under the other's MFMAs: against one workgroup of 6 blocks per CU,
// store-writing train query 87.5 -> 78.6 ms and eval query 64.0 -> 61.7 ms at 25.2M samples, bit-identical; MfmaUtil
// 38.9 -> 55.3 % / 49.4 -> 61.7 % (profiles/r04_occupancy_*.json; the clock drops ~20 %: the board's power limit).
// One 4-wave workgroup per CU: 5, 7 or 3 blocks all slower than 6 (profiles/r03l_variants_eval_sb*.json,
// r04_occupancy_ab); in the 8-wave form of the train query 7 blocks are faster than 6 (profiles/TRAIN_QUERY_FORM.md).
constexpr int EH3_SB = 3;
constexpr int EH3_WG_PER_CU = 2;
static_assert(96 % (16 * EH3_SB) == 0, "store_layer_bytes (pcnerf_internal.h) pads a chunk to whole 96-sample blocks");
// The wide geometry <NW = 8, SB = 6>: the same 96 samples per CU as ONE workgroup of 8 waves, wave w owning neuron
// blocks 2w, 2w + 1 (J = 2), so a CU streams the weight image once per 96 samples instead of twice; still two waves
// per SIMD, but the two halves no longer run independent phases.  ~140 KiB of LDS, __launch_bounds__(512, 1).
// (The store-less train query runs it with 8 blocks, 128 samples, by default: EH3_SB_WIDE8 below.)
constexpr int EH3_SB_WIDE = 6;
static_assert(96 % (16 * EH3_SB_WIDE) == 0, "store_layer_bytes pads a chunk to whole 96-sample blocks");
// k_nof_eval_h3: weight-ring slots (prefetch distance R3 - 1 k-steps of 32).  The ring index is pos % R3 with pos a
// compile-time constant at every call site, which needs every layer of a rolled layer loop to start on the same slot:
// R3 = 2 and 4 do, 3 would need the layer loops unrolled (not built).  Measurements of the geometries and ring depths:
// profiles/QUERY_GEOMETRY.md
constexpr int EH3_RING = 2;
constexpr int EH3_RING_DEEP = 4;
// The store-writing train query writes the activation store nontemporal (streamed past L2, which holds the weight
// image): -3.8 % (profiles/r03n_variants_eval_ntstore.json).  k_nof_eval_h3<true> issues the MFMAs of a product
// group neuron-block-outer, the eval query sample-block-outer: -0.9 % / -1.4 % and +4.2 % in same-process A/Bs,
// bit-identical (profiles/r03l_variants_eval_order.json, r03q_variants_eval_order_tr.json).
// Scales (eval): each layer's weights at 2^sw[L] (k_eval_wscale), each sample's B operands at the power of two
// that puts its largest |x| in [2^14, 2^15) (eh_scale; exchanged between the waves through smax), undone by one
// exact fma with the bias in the epilogue.
// TR (the train-mode query, pcnerf_nof_query_train_fused): the image holds the RAW weights (no BatchNorm fold) and
// each layer's epilogue applies its chunk's BatchNorm -- alpha = fl32(invstd) gamma, beta'' = beta - mean(W x) alpha
// from the chunk's exact batch statistics (nof_fold.hip k_tf_coeffs) -- as ONE fma per value that also moves the
// result to the next layer's operand scale: BatchNorm output k of a chunk of n samples has batch mean beta_k and
// batch variance <= gamma_k^2, so no sample exceeds sqrt(n) |gamma_k| + |beta_k| (Samuelson), and that bound fixes a
// per-layer power-of-two scale sxB[L] in advance (k_tf_coeffs): no per-sample maxima, no exchange of them between
// the waves.  Only the encoding (layers 0 and 4) keeps a per-sample scale, min(its own, sxB[3]).  blockIdx.y is the
// BatchNorm chunk, blockIdx.x the 16 EH3_SB-sample block inside it, so no block straddles two chunks.
// coef per chunk: [L][alpha 256 | beta'' 256] floats, then sxB[8] as int (TQ_COEF_FLOATS floats per chunk).
// TR with an activation store (ST; launch_train_query runs the stored chunks as their own launch, blockIdx.y + cy0 is
// the chunk): each layer's raw output W_L x + b_L (the layered kernels' stored h, nof_train.hip StoreChunk) is written
// before the BatchNorm fma, whole 32-sample tiles (the store pads a chunk to 96 samples), its raw bias from LDS
// (loaded one layer ahead): a global bias load there waited for the previous sample block's stores.  Compile-time
// store + LDS bias: store-writing query -3.3 % (profiles/r04_variants_store_query.json).
// PT (the explicit-point source, compile-time: the ray / ein forms are the code they were): `rays` holds the (total, 3)
// sample positions, read verbatim (load_point); stride, z, S and ein are not read.
template <bool TR, bool ST = false, int NW = 4, int SB = EH3_SB, int R3 = EH3_RING, bool PT = false>
__global__ __launch_bounds__(64 * NW, NW == 4 ? EH3_WG_PER_CU : 1) void k_nof_eval_h3(
                                                        const float* __restrict__ rays, int stride,
                                                        const float* __restrict__ z, int64_t total, int S,
                                                        const float* __restrict__ ein, const float* __restrict__ W,
                                                        float* __restrict__ p_out, const float* __restrict__ coef,
                                                        int64_t chunk, float* __restrict__ hst, int64_t hst_chunk,
                                                        int64_t hst_layer, int cy0) {
  static_assert(NW == 4 || NW == 8, "waves per workgroup");
  static_assert(!(PT && ST), "the activation store is not built for the point source");
  // J neuron blocks per wave, JP output k-steps per wave, WPG waves per 64-neuron group of occ_out's sum
  constexpr int NT = 64 * NW, J = 16 / NW, JP = J / 2, WPG = NW / 4, NS = 16 * SB, D3 = R3 - 1;
  constexpr bool ORD = TR;
  // DIET (the 8-block form of the 8-wave store-less train query, pcnerf_set_train_query_form 4): act + eb alone are
  // the CU's 163,840 B of LDS, so nothing else lives there -- the BatchNorm coefficients come straight from `coef`
  // (L2) into registers one k-step before each layer end, spos / sx0s sit in act behind the encoding staging area
  // (act is not written before the barrier after layer 0's MFMAs; sx0 is copied to registers before that), pdot in
  // eb behind the occ_out hand-over.  Same operands into the same fmas: same bits.
  constexpr bool DIET = TR && !ST && NW == 8 && SB == 8;
  typedef float f32x4_ __attribute__((ext_vector_type(4)));
  __shared__ eh_f16x8 act[8][SB][2][64];
  __shared__ eh_f16x8 eb[2][SB][2][64];   // the encoding's B operands at the layer-0 scale (sx0)
  static_assert(!DIET || sizeof(act) + sizeof(eb) == 163840, "the 8-block form: act + eb are the CU's LDS");
  __shared__ int sx0s[NS];
  __shared__ __attribute__((aligned(16))) float sbias[(TR ? 16 : 8) * 256];
  __shared__ float emax[NS];
  __shared__ float smax[NW][NS];   // (eval)
  __shared__ float pdot[4][NS];
  __shared__ float spos[NS][3];
  // TR with the store: the raw biases of two consecutive layers (slot L & 1), each loaded one layer ahead
  __shared__ __attribute__((aligned(16))) float sbraw[TR ? 2 : 1][TR ? 256 : 4];
  // DIET: [sample][65] encoding staging | spos | sx0s in act, hand | pdot in eb; sbias is not referenced
  float* const actf = reinterpret_cast<float*>(&act[0][0][0][0]);
  float* const ebf = reinterpret_cast<float*>(&eb[0][0][0][0]);
  float (*const sposv)[3] = DIET ? reinterpret_cast<float (*)[3]>(actf + NS * 65) : spos;
  int* const sx0v = DIET ? reinterpret_cast<int*>(actf + NS * 68) : sx0s;
  float (*const pdotv)[NS] = DIET ? reinterpret_cast<float (*)[NS]>(ebf + 4 * SB * 64) : pdot;
  const int t = threadIdx.x, w = __builtin_amdgcn_readfirstlane(t >> 6), lane = t & 63, g = lane >> 4, li = lane & 15;
  const int cy = (int)blockIdx.y + cy0;   // the BatchNorm chunk
  const int64_t cb = TR ? (int64_t)cy * chunk : 0;
  const int64_t s0 = cb + (int64_t)blockIdx.x * NS;
  const int64_t send = TR ? (cb + chunk < total ? cb + chunk : total) : total;
  if (s0 >= send) return;   // (the last chunk's surplus blocks; uniform over the block, before any barrier)
  constexpr bool storing = TR && ST;
  float rz = 0.0f, rr[6] = {};
  if constexpr (PT) {
    if (t < NS) {
      int64_t gs = s0 + t;
      if (gs >= send) gs = send - 1;
      float p[3];
      load_point(rays, gs, p);
#pragma unroll
      for (int m = 0; m < 3; ++m) rr[m] = p[m];
    }
  } else if (!ein && t < NS) {
    int64_t gs = s0 + t;
    if (gs >= send) gs = send - 1;
    const float* r = rays + ray_of(gs, S) * stride;
    rz = z[gs];
#pragma unroll
    for (int m = 0; m < 6; ++m) rr[m] = r[m];
  }
  const eh_f16x8* __restrict__ img = reinterpret_cast<const eh_f16x8*>(W + OFF_EH);
  int sw[8];
#pragma unroll
  for (int L = 0; L < 8; ++L) sw[L] = __builtin_amdgcn_readfirstlane(reinterpret_cast<const int*>(W + OFF_EH_SW)[L]);
  int sxB[8];
  if (TR) {
    const int* cs = reinterpret_cast<const int*>(coef + cy * (size_t)TQ_COEF_FLOATS + 16 * 256);
#pragma unroll
    for (int L = 0; L < 8; ++L) sxB[L] = __builtin_amdgcn_readfirstlane(L < 7 ? cs[L] : 0);
  }
  // this wave's A operands of k-step gk: neuron blocks J w + j, parts hi / mid
  auto load_w = [&](eh_f16x8 (&d)[J][2], int gk) __attribute__((always_inline)) {
    // (k-steps past the end reload the last one: unconditional loads keep the ring's registers statically known to
    // the waitcnt pass -- a conditional load made it wait for every load in flight)
    gk = gk < EH3_KSTEPS ? gk : EH3_KSTEPS - 1;
#pragma unroll
    for (int j = 0; j < J; ++j)
#pragma unroll
      for (int p = 0; p < 2; ++p) d[j][p] = img[((size_t)(gk * 16 + J * w + j) * 2 + p) * 64 + lane];
  };
  eh_f16x8 wr[R3][J][2];
#pragma unroll
  for (int k = 0; k < D3; ++k) load_w(wr[k], k);
  if (storing && (NT == 256 || t < 256)) {
    sbraw[0][t] = W[OFF_BIAS + t];
    sbraw[TR ? 1 : 0][t] = W[OFF_BIAS + 256 + t];
  }
  if (DIET) {
    // (no coefficient image in LDS: coef_load / epi_tr below)
  } else if (TR) {
    const f32x4_* cf = reinterpret_cast<const f32x4_*>(coef + cy * (size_t)TQ_COEF_FLOATS);
    constexpr int CM = 16 * 256 / 4 / NT;
    f32x4_ cv[CM];
#pragma unroll
    for (int m = 0; m < CM; ++m) cv[m] = cf[t + NT * m];
#pragma unroll
    for (int m = 0; m < CM; ++m) {
      const int i = 4 * (t + NT * m), L = i >> 9, isb = (i >> 8) & 1;
      const int sxo = sxB[L], sxi = (L == 0 || L == 4) ? 0 : sxB[L - 1];
      const int e = isb ? sxo : sxo - sw[L] - sxi;
      reinterpret_cast<f32x4_*>(sbias)[t + NT * m] =
          f32x4_{ldexpf(cv[m][0], e), ldexpf(cv[m][1], e), ldexpf(cv[m][2], e), ldexpf(cv[m][3], e)};
    }
  } else {
    for (int i = t; i < 8 * 256 / 4; i += NT)
      reinterpret_cast<f32x4_*>(sbias)[i] = reinterpret_cast<const f32x4_*>(W + OFF_BIAS)[i];
  }
  float* const encf = reinterpret_cast<float*>(&act[0][0][0][0]);   // [sample][65]
  static_assert(sizeof(act) >= NS * (65 + (DIET ? 4 : 0)) * sizeof(float), "encoding staging area (DIET: + spos, sx0s)");
  if (PT || !ein) {
    if (t < NS) {
      float p[3];
      if constexpr (PT) p[0] = rr[0], p[1] = rr[1], p[2] = rr[2];
      else sample_point(rr, rz, p);
#pragma unroll
      for (int m = 0; m < 3; ++m) {
        sposv[t][m] = p[m];
        encf[t * 65 + m] = p[m];
      }
      encf[t * 65 + 63] = 0.0f;
    }
    __syncthreads();
    for (int i = t; i < NS * 30; i += NT) {
      const int sm = i / 30, r = i - 30 * sm, k = r / 3, m = r - 3 * k;
      float sv, cv;
      sincosf((float)(1 << k) * sposv[sm][m], &sv, &cv);
      encf[sm * 65 + 3 + 6 * k + m] = sv;
      encf[sm * 65 + 6 + 6 * k + m] = cv;
    }
    __syncthreads();
  }
  if (t < NS) {   // one sample's encoding per thread, stored in B order
    float f[64];
    if (!PT && ein) {
      int64_t gs = s0 + t;
      if (gs >= send) gs = send - 1;
#pragma unroll
      for (int k = 0; k < 63; ++k) f[k] = ein[gs * 63 + k];
      f[63] = 0.0f;
    } else {
#pragma unroll
      for (int k = 0; k < 64; ++k) f[k] = encf[t * 65 + k];
    }
    float m = 0.0f;
#pragma unroll
    for (int k = 0; k < 63; ++k) m = fmaxf(m, fabsf(f[k]));
    int sx0 = eh_scale(m);
    if (TR && sxB[3] < sx0) sx0 = sxB[3];
    const float xs = ldexpf(1.0f, sx0);
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int gg = 0; gg < 4; ++gg) {
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = f[32 * s + 8 * gg + e] * xs;
        eh_f16x8 hi, mid;
        eh_split8(v, hi, mid);
        eb[s][t >> 4][0][(t & 15) + 16 * gg] = hi;
        eb[s][t >> 4][1][(t & 15) + 16 * gg] = mid;
      }
    if (!TR) emax[t] = m;
    sx0v[t] = sx0;
  }
  __syncthreads();
  int sxl[SB];   // the per-sample scale of the current layer's B operands (this lane's sample of each block)
#pragma unroll
  for (int sb = 0; sb < SB; ++sb) sxl[sb] = sx0v[16 * sb + li];
  int sx0l[DIET ? SB : 1];   // DIET: sx0s leaves LDS with act's first write, so every lane keeps its own
  if (DIET) {
#pragma unroll
    for (int sb = 0; sb < SB; ++sb) sx0l[sb] = sxl[sb];
  }
  // DIET: this lane's BatchNorm coefficients of the layer that ends next (alpha, beta'' of its J x 4 neurons, raw),
  // loaded from coef one k-step before the layer end; epi_tr scales them as the other forms' prologue does
  f32x4_ cfa[J], cfb[J];
  auto coef_load = [&](int L) __attribute__((always_inline)) {
    if constexpr (DIET) {
      const float* c = coef + cy * (size_t)TQ_COEF_FLOATS + 512 * L + 16 * J * w + 4 * g;
#pragma unroll
      for (int j = 0; j < J; ++j) {
        cfa[j] = *reinterpret_cast<const f32x4_*>(c + 16 * j);
        cfb[j] = *reinterpret_cast<const f32x4_*>(c + 256 + 16 * j);
      }
    }
  };
  f32x4_ acc[J][SB];
  int gk = 0;
  // one encoding k-step (layers 0 and 4)
  auto kstep_enc = [&](int s, int pos, bool first) __attribute__((always_inline)) {
    load_w(wr[(pos + D3) % R3], gk + D3);
    const eh_f16x8 (&wc)[J][2] = wr[pos % R3];
    eh_f16x8 bh[SB], bm[SB];
#pragma unroll
    for (int sb = 0; sb < SB; ++sb) {
      bh[sb] = eb[s][sb][0][lane];
      bm[sb] = eb[s][sb][1][lane];
      const int d = TR ? 0 : sxl[sb] - sx0s[16 * sb + li];
      if (d != 0) {   // eval layer 4: the 22-bit encoding (hi + mid, exact in fp32) re-split at the shared scale
        const float xs = ldexpf(1.0f, d);
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = ((float)bh[sb][e] + (float)bm[sb][e]) * xs;
        eh_split8(v, bh[sb], bm[sb]);
      }
    }
#pragma unroll
    for (int o1 = 0; o1 < (ORD ? J : SB); ++o1)
#pragma unroll
      for (int o2 = 0; o2 < (ORD ? SB : J); ++o2) {
        const int sb = ORD ? o2 : o1, j = ORD ? o1 : o2;
        acc[j][sb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wc[j][0], bm[sb], first ? f32x4_{} : acc[j][sb], 0, 0, 0);
      }
#pragma unroll
    for (int o1 = 0; o1 < (ORD ? J : SB); ++o1)
#pragma unroll
      for (int o2 = 0; o2 < (ORD ? SB : J); ++o2) {
        const int sb = ORD ? o2 : o1, j = ORD ? o1 : o2;
        acc[j][sb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wc[j][0], bh[sb], acc[j][sb], 0, 0, 0);
      }
#pragma unroll
    for (int o1 = 0; o1 < (ORD ? J : SB); ++o1)
#pragma unroll
      for (int o2 = 0; o2 < (ORD ? SB : J); ++o2) {
        const int sb = ORD ? o2 : o1, j = ORD ? o1 : o2;
        acc[j][sb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wc[j][1], bh[sb], acc[j][sb], 0, 0, 0);
      }
    ++gk;
  };
  // the 8 hidden k-steps of a layer, software-pipelined: per k-step the products run in the order Wh.xm, Wh.xh,
  // Wm.xh, and k-step s + 1's xm is read from LDS once Wh.xm of s is issued, its xh once Wm.xh of s is -- every LDS
  // read has at least 24 MFMAs in flight to cover it
  auto hidden_ksteps = [&](int pos0, bool first, int L) __attribute__((always_inline)) {
    eh_f16x8 bh[SB], bm[SB];
#pragma unroll
    for (int sb = 0; sb < SB; ++sb) {
      bm[sb] = act[0][sb][1][lane];
      bh[sb] = act[0][sb][0][lane];
    }
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      const int pos = pos0 + s;
      if (s == 7) coef_load(L);
      load_w(wr[(pos + D3) % R3], gk + D3);
      const eh_f16x8 (&wc)[J][2] = wr[pos % R3];
#pragma unroll
      for (int o1 = 0; o1 < (ORD ? J : SB); ++o1)
#pragma unroll
        for (int o2 = 0; o2 < (ORD ? SB : J); ++o2) {
          const int sb = ORD ? o2 : o1, j = ORD ? o1 : o2;
          acc[j][sb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wc[j][0], bm[sb], (first && s == 0) ? f32x4_{} : acc[j][sb], 0, 0, 0);
        }
      __builtin_amdgcn_sched_barrier(0);
      if (s + 1 < 8) {
#pragma unroll
        for (int sb = 0; sb < SB; ++sb) bm[sb] = act[s + 1][sb][1][lane];
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int o1 = 0; o1 < (ORD ? J : SB); ++o1)
#pragma unroll
        for (int o2 = 0; o2 < (ORD ? SB : J); ++o2) {
          const int sb = ORD ? o2 : o1, j = ORD ? o1 : o2;
          acc[j][sb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wc[j][0], bh[sb], acc[j][sb], 0, 0, 0);
        }
#pragma unroll
      for (int o1 = 0; o1 < (ORD ? J : SB); ++o1)
#pragma unroll
        for (int o2 = 0; o2 < (ORD ? SB : J); ++o2) {
          const int sb = ORD ? o2 : o1, j = ORD ? o1 : o2;
          acc[j][sb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wc[j][1], bh[sb], acc[j][sb], 0, 0, 0);
        }
      __builtin_amdgcn_sched_barrier(0);
      if (s + 1 < 8) {
#pragma unroll
        for (int sb = 0; sb < SB; ++sb) bh[sb] = act[s + 1][sb][0][lane];
      }
      __builtin_amdgcn_sched_barrier(0);
      ++gk;
    }
  };
  // eval epilogue phase 1: acc <- fl(acc 2^-(sw + sx) + bias), this wave's per-sample maxima -> smax[w]
  auto epi1 = [&](int L) __attribute__((always_inline)) {
#pragma unroll
    for (int sb = 0; sb < SB; ++sb) {
      const float us = ldexpf(1.0f, -(sw[L] + sxl[sb]));
      float m = 0.0f;
#pragma unroll
      for (int j = 0; j < J; ++j) {
        const f32x4_ b = *reinterpret_cast<const f32x4_*>(sbias + 256 * L + 16 * J * w + 16 * j + 4 * g);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float v = __builtin_fmaf(acc[j][sb][q], us, b[q]);
          acc[j][sb][q] = v;
          m = fmaxf(m, fabsf(v));
        }
      }
      m = fmaxf(m, __shfl_xor(m, 16, 64));
      m = fmaxf(m, __shfl_xor(m, 32, 64));
      if (g == 0) smax[w][16 * sb + li] = m;
    }
  };
  // this wave's outputs as the next layer's B operands (k-steps JP w .. JP w + JP - 1), at scale xs per sample block
  auto split_out = [&](const float (&xs)[SB], auto SC) {
#pragma unroll
    for (int sb = 0; sb < SB; ++sb)
#pragma unroll
      for (int jp = 0; jp < JP; ++jp) {
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float a = acc[2 * jp + (e >> 2)][sb][e & 3];
          v[e] = decltype(SC)::value ? a * xs[sb] : a;
        }
        eh_f16x8 hi, mid;
        eh_split8(v, hi, mid);
        act[JP * w + jp][sb][0][lane] = hi;
        act[JP * w + jp][sb][1][lane] = mid;
      }
  };
  auto epi2 = [&](bool with_e) __attribute__((always_inline)) {
    float xs[SB];
#pragma unroll
    for (int sb = 0; sb < SB; ++sb) {
      const int sm = 16 * sb + li;
      float m = fmaxf(fmaxf(smax[0][sm], smax[1][sm]), fmaxf(smax[2][sm], smax[3][sm]));
#pragma unroll
      for (int k = 4; k < NW; ++k) m = fmaxf(m, smax[k][sm]);   // (a maximum: the order is free)
      if (with_e) m = fmaxf(m, emax[sm]);
      sxl[sb] = eh_scale(m);
      xs[sb] = ldexpf(1.0f, sxl[sb]);
    }
    split_out(xs, std::true_type{});
  };
  // TR: the activation store (the layered kernels' [32-sample tile][k-group][lane][4] layout): accumulator
  // acc[j][sb] of lane l is neurons 64w + 16j + 4g .. + 3 = k-group 8w + 2j + (g >> 1), half g & 1, of sample
  // 16(q & 1) + (l & 15) of tile q >> 1, q = SB blockIdx.x + sb the 16-sample block within the chunk
  auto store_raw = [&](int L, int sb, int j, float sc) __attribute__((always_inline)) {
    const int64_t q = (int64_t)blockIdx.x * SB + sb, tile = q >> 1;
    const int n0 = 16 * J * w + 16 * j + 4 * g;
    const f32x4_ b = *reinterpret_cast<const f32x4_*>(&sbraw[TR ? L & 1 : 0][TR ? n0 : 0]);
    const f32x4_ v = {acc[j][sb][0] * sc + b[0], acc[j][sb][1] * sc + b[1], acc[j][sb][2] * sc + b[2],
                      acc[j][sb][3] * sc + b[3]};
    const int sl = 16 * (int)(q & 1) + li + 32 * (g & 1);
    // a uniform layer base and a 32-bit byte offset (launch_train_query checks a layer's region is < 4 GiB): the
    // stores take the scalar-base form, one offset register per sample block
    char* const hb = reinterpret_cast<char*>(hst + (int64_t)cy * hst_chunk + (int64_t)L * hst_layer);
    const uint32_t off = ((uint32_t)tile * 32u + (uint32_t)(2 * J * w + (g >> 1))) * 1024u + (uint32_t)sl * 16u +
                         (uint32_t)j * 2048u;
    __builtin_nontemporal_store(v, reinterpret_cast<f32x4_*>(hb + off));
  };
  auto epi_tr = [&](int L, auto PS) __attribute__((always_inline)) {
    constexpr bool ps = decltype(PS)::value;
    if constexpr (DIET) {
      // the coefficients at the scales the other forms' prologue gives them (uniform exponents, ldexpf exact), once
      // per layer: they depend on j only
      const int ea = sxB[L] - sw[L] - ((L == 0 || L == 4) ? 0 : sxB[L > 0 ? L - 1 : 0]), ebt = sxB[L];
      f32x4_ a[J], b[J];
#pragma unroll
      for (int j = 0; j < J; ++j)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          a[j][q] = ldexpf(cfa[j][q], ea);
          b[j][q] = ldexpf(cfb[j][q], ebt);
        }
#pragma unroll
      for (int sb = 0; sb < SB; ++sb) {
        const float us = ps ? ldexpf(1.0f, -sxl[sb]) : 1.0f;
#pragma unroll
        for (int j = 0; j < J; ++j)
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            float v = acc[j][sb][q];
            if (ps) v *= us;
            acc[j][sb][q] = __builtin_fmaf(v, a[j][q], b[j][q]);
          }
      }
      return;
    }
#pragma unroll
    for (int sb = 0; sb < SB; ++sb) {
      const float us = ps ? ldexpf(1.0f, -sxl[sb]) : 1.0f;
      if (storing) {
        const float sc = ldexpf(1.0f, -(sw[L] + (ps ? sxl[sb] : (L > 0 ? sxB[L - 1] : 0))));
#pragma unroll
        for (int j = 0; j < J; ++j) store_raw(L, sb, j, sc);
      }
#pragma unroll
      for (int j = 0; j < J; ++j) {
        const int nb = 16 * J * w + 16 * j + 4 * g;
        const f32x4_ a = *reinterpret_cast<const f32x4_*>(sbias + 512 * L + nb);
        const f32x4_ b = *reinterpret_cast<const f32x4_*>(sbias + 512 * L + 256 + nb);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          float v = acc[j][sb][q];
          if (ps) v *= us;
          acc[j][sb][q] = __builtin_fmaf(v, a[q], b[q]);
        }
      }
    }
  };
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    if (s == 1) coef_load(0);
    kstep_enc(s, s, s == 0);
  }
  if (TR) {
    epi_tr(0, std::true_type{});
    float xs[SB];
#pragma unroll
    for (int sb = 0; sb < SB; ++sb) {
      sxl[sb] = sxB[0];
      xs[sb] = 1.0f;
    }
    __syncthreads();
    split_out(xs, std::false_type{});
    __syncthreads();
  } else {
    epi1(0);
    __syncthreads();
    epi2(false);
    __syncthreads();
  }
  // the next layer's raw bias, loaded at the start of layer L (bnext) and written to its slot before L's epilogue
  float bnext = 0.0f;
  auto bias_load = [&](int L) __attribute__((always_inline)) {
    if (storing && L < 7 && (NT == 256 || t < 256)) bnext = W[OFF_BIAS + 256 * (L + 1) + t];
  };
  auto layer_end = [&](int L) __attribute__((always_inline)) {
    if (TR) {
      if (storing && L < 7 && (NT == 256 || t < 256)) sbraw[TR ? (L + 1) & 1 : 0][TR ? t : 0] = bnext;
      if (L == 4) epi_tr(4, std::true_type{});
      else epi_tr(L, std::false_type{});
      if (L < 7) {
        float xs[SB];
#pragma unroll
        for (int sb = 0; sb < SB; ++sb) {
          const int sx0 = DIET ? sx0l[sb] : sx0s[16 * sb + li];
          sxl[sb] = L == 3 ? sx0 : sxB[L];
          xs[sb] = ldexpf(1.0f, sx0 - sxB[3]);
        }
        __syncthreads();
        if (L == 3) split_out(xs, std::true_type{});
        else split_out(xs, std::false_type{});
        __syncthreads();
      }
    } else {
      epi1(L);
      __syncthreads();
      if (L < 7) {
        epi2(L == 3);
        __syncthreads();
      }
    }
  };
  // ring slots: layer starts 0, 2, 10, 18, 26 (+2 encoding k-steps), 36, 44, 52 -- every call site's position is a
  // compile-time constant mod the ring
  static_assert(eh3_start(1) % R3 == eh3_start(2) % R3 && eh3_start(2) % R3 == eh3_start(3) % R3, "ring slots");
  static_assert((eh3_start(4) + 2) % R3 == eh3_start(5) % R3 && eh3_start(5) % R3 == eh3_start(6) % R3 &&
                eh3_start(6) % R3 == eh3_start(7) % R3, "ring slots");
#pragma unroll 1
  for (int L = 1; L <= 3; ++L) {
    if (TR) bias_load(L);
    hidden_ksteps(eh3_start(1) % R3, true, L);
    layer_end(L);
  }
  if (TR) bias_load(4);
#pragma unroll
  for (int s = 0; s < 2; ++s) kstep_enc(s, eh3_start(4) % R3 + s, s == 0);
  hidden_ksteps((eh3_start(4) + 2) % R3, false, 4);
  layer_end(4);
#pragma unroll 1
  for (int L = 5; L <= 7; ++L) {
    if (TR) bias_load(L);
    hidden_ksteps(eh3_start(5) % R3, true, L);
    layer_end(L);
  }
  // occ_out: each 64-neuron group's fma chain per lane and sample block (j, q ascending), the two cross-lane adds,
  // then the 4 group sums in order.  NW = 4: wave w is group w.  NW = 8: waves 2p, 2p + 1 are group p -- the even
  // wave runs the chain's first half (neuron blocks 4p, 4p + 1) and hands its running value per lane to the odd wave
  // through LDS (eb: last read in layer 4, two or more barriers ago), which continues it: the same fmas in the same
  // order as the 4-wave form
  auto occ_chain = [&](int sb, float part) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < J; ++j) {
      const f32x4_ wv = *reinterpret_cast<const f32x4_*>(W + OFF_WOUT + 16 * J * w + 16 * j + 4 * g);
#pragma unroll
      for (int q = 0; q < 4; ++q) part = fmaf(wv[q], acc[j][sb][q], part);
    }
    return part;
  };
  float (*const hand)[SB][64] = reinterpret_cast<float (*)[SB][64]>(&eb[0][0][0][0]);
  static_assert(sizeof(eb) >= (4 * SB * 64 + (DIET ? 4 * NS : 0)) * sizeof(float), "occ_out handover area (DIET: + pdot)");
  if (WPG == 2) {
    if (!(w & 1)) {
#pragma unroll
      for (int sb = 0; sb < SB; ++sb) hand[w >> 1][sb][lane] = occ_chain(sb, 0.0f);
    }
    __syncthreads();
  }
  if (WPG == 1 || (w & 1)) {
#pragma unroll
    for (int sb = 0; sb < SB; ++sb) {
      float part = occ_chain(sb, WPG == 1 ? 0.0f : hand[w >> 1][sb][lane]);
      part += __shfl_xor(part, 16, 64);
      part += __shfl_xor(part, 32, 64);
      if (g == 0) pdotv[w / WPG][16 * sb + li] = part;
    }
  }
  __syncthreads();
  if (t < NS && s0 + t < send) {
    const float logit = ((pdotv[0][t] + pdotv[1][t]) + (pdotv[2][t] + pdotv[3][t])) + W[OFF_BOUT];
    p_out[s0 + t] = sigmoid_ref(logit);
  }
}

// Eval-mode MLP arithmetic: 0 = fp32 MFMA (k_nof_eval), 1 = split fp16, 3 products (k_nof_eval_h3, default).
static int g_eval_math = 1;

// Geometry of k_nof_eval_h3 for the eval query and the store-less train query (pcnerf_set_query_geometry):
// bit 0 = the 8-wave workgroup of 96 samples, bit 1 = the 4-slot weight ring; -1 = each form's measured default.
// Every geometry computes the same bits (tests/test_query_geometry_gpu.py).
static int g_query_geometry = -1;
// The defaults, from the interleaved A/B against the parent commit (profiles/QUERY_GEOMETRY.md): the train query
// takes the 8-wave form (config 2 forward 83.31 -> 80.02 ms, L2 read requests halved, clock up), the eval query stays
// on the 4-wave form (8 waves: +0.3 %, inside the spread); the 4-slot ring lost in both geometries and both queries.
constexpr int EH3_GEOM_EVAL = 0, EH3_GEOM_TRAIN = 1;
// Form of the store-less train query where it runs in the 8-wave geometry with the 2-slot ring (geometry -1 or 1;
// pcnerf_set_train_query_form): 0 = 6 sample blocks (96 samples per pass over the weight image), 2 = 7 sample blocks
// (112 samples per pass: 6/7 of the L2 weight stream per sample; 163,328 B of LDS -- the train form without the store
// allocates no smax / emax / sbraw, so it just fits the CU's 160 KiB; 213 VGPRs; config 2 forward 77.63 -> 76.21 ms),
// 4 = 8 sample blocks (128 samples per pass: 7/8 of form 2's stream; act + eb are the CU's whole 163,840 B of LDS, the
// small arrays and the coefficient image live elsewhere -- DIET in the kernel; 250 VGPRs, no spills); -1 = the
// measured default, form 4 (config 2 forward 76.84 -> 75.00 ms, profiles/TRAIN_QUERY_FORM.md).  No 9th block fits:
// the weight-stream lever ends here in this decomposition.  1 was the half-skewed form: measured slower, not built
// (HISTORY.md); 3 was never built.  Same bits in every form (tests/test_train_query_form_gpu.py,
// tests/test_train_query_form8_gpu.py).
static int g_train_query_form = -1;
constexpr int EH3_TRAIN_FORM = 4;
constexpr int EH3_SB_WIDE7 = 7;
constexpr int EH3_SB_WIDE8 = 8;

// Form 4's 160 KiB of static LDS against the device's limit, asked once per process and point source: where it cannot
// be launched the default falls back to form 2 (a message in pcnerf_last_error), and selecting 4 is an error.
template <bool PT>
static bool form8_launchable() {
  static const bool ok = [] {
    hipFuncAttributes fa;
    int dev = 0, lim = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&lim, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) != hipSuccess ||
        hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(
                                      &k_nof_eval_h3<true, false, 8, EH3_SB_WIDE8, EH3_RING, PT>)) != hipSuccess) {
      (void)hipGetLastError();
      return false;
    }
    return fa.sharedSizeBytes <= (size_t)lim;
  }();
  return ok;
}

// launches k_nof_eval_h3<TR, false> in geometry geom: `rows` grid rows (BatchNorm chunks) of `span` samples each
// (PT: the point source, the positions in the kernel's `rays` argument)
template <bool TR, bool PT, typename... Args>
static void launch_h3(int geom, int64_t span, unsigned rows, hipStream_t s, Args... args) {
  const bool wide = geom & 1, deep = geom & 2;
  if constexpr (TR) {   // the 7- and 8-block forms of the 8-wave train query (pcnerf_set_train_query_form)
    int form = g_train_query_form < 0 ? EH3_TRAIN_FORM : g_train_query_form;
    if (wide && !deep && form == 4 && !form8_launchable<PT>()) {
      if (g_train_query_form == 4)
        throw std::runtime_error("train query: form 4 needs 163,840 B of LDS per workgroup, more than this device "
                                 "gives");
      set_error("train query: form 4 (163,840 B of LDS per workgroup) cannot be launched on this device; the "
                "default falls back to form 2");
      form = 2;
    }
    if (wide && !deep && form == 4) {
      const int64_t ns8 = 16 * EH3_SB_WIDE8;
      hipLaunchKernelGGL((k_nof_eval_h3<true, false, 8, EH3_SB_WIDE8, EH3_RING, PT>),
                         dim3((unsigned)((span + ns8 - 1) / ns8), rows), dim3(512), 0, s, args...);
      return;
    }
    if (wide && !deep && form == 2) {
      const int64_t ns7 = 16 * EH3_SB_WIDE7;
      hipLaunchKernelGGL((k_nof_eval_h3<true, false, 8, EH3_SB_WIDE7, EH3_RING, PT>),
                         dim3((unsigned)((span + ns7 - 1) / ns7), rows), dim3(512), 0, s, args...);
      return;
    }
  }
  const int64_t ns = 16 * (wide ? EH3_SB_WIDE : EH3_SB);
  const dim3 grid((unsigned)((span + ns - 1) / ns), rows), block(wide ? 512 : 256);
  if (wide && deep)
    hipLaunchKernelGGL((k_nof_eval_h3<TR, false, 8, EH3_SB_WIDE, EH3_RING_DEEP, PT>), grid, block, 0, s, args...);
  else if (wide)
    hipLaunchKernelGGL((k_nof_eval_h3<TR, false, 8, EH3_SB_WIDE, EH3_RING, PT>), grid, block, 0, s, args...);
  else if (deep)
    hipLaunchKernelGGL((k_nof_eval_h3<TR, false, 4, EH3_SB, EH3_RING_DEEP, PT>), grid, block, 0, s, args...);
  else
    hipLaunchKernelGGL((k_nof_eval_h3<TR, false, 4, EH3_SB, EH3_RING, PT>), grid, block, 0, s, args...);
}

// pts != NULL: the explicit-point source (eval math 1 only; the caller checks)
static void launch_eval(const float* rays, int stride, const float* z, int64_t total, int S, const float* ein,
                        const float* W, float* p_out, hipStream_t s, const float* pts = nullptr) {
  if (pts) {
    if (g_eval_math != 1) throw std::runtime_error("point query: needs eval math 1 (split fp16)");
    launch_h3<false, true>(g_query_geometry < 0 ? EH3_GEOM_EVAL : g_query_geometry, total, 1u, s, pts, 3,
                           (const float*)nullptr, total, 1, (const float*)nullptr, W, p_out, (const float*)nullptr,
                           (int64_t)0, (float*)nullptr, (int64_t)0, (int64_t)0, 0);
  } else if (g_eval_math == 1) {
    launch_h3<false, false>(g_query_geometry < 0 ? EH3_GEOM_EVAL : g_query_geometry, total, 1u, s, rays, stride, z,
                            total, S, ein, W, p_out, (const float*)nullptr, (int64_t)0, (float*)nullptr, (int64_t)0,
                            (int64_t)0, 0);
  } else {
    const int64_t blocks = ((total + 31) / 32 + 3) / 4;
    hipLaunchKernelGGL(k_nof_eval, dim3((unsigned)blocks), dim3(256), 0, s, rays, stride, z, total, S, ein, W,
                       p_out);
  }
}

__global__ void k_embed(const float* __restrict__ pts, int64_t n, float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float p[3] = {pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]};
  float e0[32], e1[32];
  encode_half(p, 0, e0);
  encode_half(p, 1, e1);
  float* o = out + 63 * i;
#pragma unroll
  for (int t = 0; t < 32; ++t) {
    o[2 * t] = e0[t];
    if (2 * t + 1 < 63) o[2 * t + 1] = e1[t];
  }
}

// ---------------------------------------------------------------------------------- exact affine fold
// Optional eval fast path: every LeakyReLU(True) of NOF is the identity (negative_slope = True
// = 1.0, models.py:72,152,232) and eval-mode BatchNorm is affine per feature, so the whole eval network is
// sigmoid(a . e + c) with a in R^63 (models.py:44-123, 183-203).  k_fold_eval composes it backwards from occ_out
// in float64: with v the coefficients of h_L, h_L = alpha (W_L x + b_L) + beta gives c += v.(alpha b_L + beta),
// v <- (v alpha) W_L (the skip layer 4 splits into its encoding and h_3 columns).  fold[0..62] = a, fold[63] = c.
// The per-sample query is then the encoding, 63 float64 FMAs and the sigmoid (no MLP).  Rounding differs from
// the layer-by-layer fp32 network (folded vs unfolded: ~1e-7 relative logit), so this path is
// opt-in and reported separately.
// sum_{n < 64} va[n] * w[n * ld] in float64, the 64 loads issued in two batches of 32 before any use (one
// workgroup runs the whole fold, so load latency, not bandwidth, sets its time)
__device__ __forceinline__ double gemv_slice(const float* __restrict__ w, int ld, const double* __restrict__ va) {
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int b = 0; b < 64; b += 32) {
    float x[32];
#pragma unroll
    for (int j = 0; j < 32; ++j) x[j] = w[(size_t)(b + j) * ld];
#pragma unroll
    for (int j = 0; j < 32; ++j) acc[j & 3] += va[b + j] * (double)x[j];
  }
  return (acc[0] + acc[1]) + (acc[2] + acc[3]);
}

__global__ __launch_bounds__(1024) void k_fold_eval(NofParamsDev P, double* __restrict__ fold) {
  // thread (t, sl): output column t, input rows n in [64 sl, 64 sl + 64) of each GEMV (16 loads in flight),
  // the four slices summed in a fixed order through LDS
  __shared__ double va[256];
  __shared__ double red[4];
  __shared__ double ps[2][4][256];
  const int tid = threadIdx.x, t = tid & 255, sl = tid >> 8;
  double v = (double)P.out_w[t];   // meaningful in slice 0
  double ae = 0.0;                 // slice 0, t < 63: coefficient of encoding feature t
  double c = (double)P.out_b[0];
  for (int L = 7; L >= 0; --L) {
    const int in_f = L == 0 ? 63 : L == 4 ? 319 : 256;
    double cb = 0.0;
    if (sl == 0) {
      const double alpha = (double)P.bn_w[L][t] / sqrt((double)P.bn_rv[L][t] + (double)P.eps);
      const double beta = (double)P.bn_b[L][t] - (double)P.bn_rm[L][t] * alpha;
      cb = v * (alpha * (double)P.lin_b[L][t] + beta);
      va[t] = v * alpha;
      const double w = wave_sum_d(cb);
      if ((t & 63) == 0) red[t >> 6] = w;
    }
    __syncthreads();
    c += (red[0] + red[1]) + (red[2] + red[3]);
    const float* __restrict__ W = P.lin_w[L];
    const int n0 = 64 * sl;
    double ea = 0.0, ha = 0.0;
    if ((L == 0 || L == 4) && t < 63) {
      ea = gemv_slice(W + (size_t)n0 * in_f + t, in_f, va + n0);
    }
    if (L != 0) {
      const int off = L == 4 ? 63 : 0;
      ha = gemv_slice(W + (size_t)n0 * in_f + off + t, in_f, va + n0);
    }
    ps[0][sl][t] = ea;
    ps[1][sl][t] = ha;
    __syncthreads();
    if (sl == 0) {
      ae += (ps[0][0][t] + ps[0][1][t]) + (ps[0][2][t] + ps[0][3][t]);
      if (L != 0) v = (ps[1][0][t] + ps[1][1][t]) + (ps[1][2][t] + ps[1][3][t]);
    }
    __syncthreads();
  }
  if (sl == 0 && t < 63) fold[t] = ae;
  if (sl == 0 && t == 63) fold[63] = c;
}

// one thread per sample: p = sigmoid(fl32(a . e + c)); ein != NULL reads the (total, 63) embedding instead.
// MODE 0: one coefficient set (eval fold); the train fold has one set per BatchNorm chunk of `chunk` samples:
// MODE 1 (chunk >= 256: a block spans at most two chunks) stages both in LDS, MODE 2 (small chunks) reads them
// from global memory per sample.
template <int MODE>
__global__ __launch_bounds__(256) void k_nof_eval_fold(const float* __restrict__ rays, int stride,
                                                       const float* __restrict__ z, int64_t total, int S,
                                                       const float* __restrict__ ein, const double* __restrict__ fold,
                                                       int64_t chunk, int64_t nfold, float* __restrict__ p_out) {
  __shared__ double a2[2][64];
  const int64_t gb = (int64_t)blockIdx.x * blockDim.x;
  const int64_t cb = MODE == 1 ? gb / chunk : 0;
  if (MODE != 2 && threadIdx.x < (MODE == 1 ? 128 : 64)) {
    int64_t cc = cb + (threadIdx.x >> 6);
    if (cc >= nfold) cc = nfold - 1;
    a2[threadIdx.x >> 6][threadIdx.x & 63] = fold[cc * 64 + (threadIdx.x & 63)];
  }
  __syncthreads();
  const int64_t g = gb + threadIdx.x;
  if (g >= total) return;
  const double* __restrict__ a = a2[0];
  if (MODE == 1) a = a2[g / chunk - cb];
  if (MODE == 2) a = fold + 64 * (g / chunk);
  double acc = a[63];
  if (ein) {
    const float* e = ein + g * 63;
#pragma unroll
    for (int f = 0; f < 63; ++f) acc += a[f] * (double)e[f];
  } else {
    // the Embedding's 63 features (encode_half's arithmetic, each sincosf once) straight into the dot product
    float p[3];
    sample_point(rays + ray_of(g, S) * stride, z[g], p);
    double unused[3];
    acc += fold_dot<true, false>(p, a, unused);
  }
  p_out[g] = sigmoid_ref((float)acc);
}

// ---- the train-mode query (nof_fold.hip pcnerf_nof_query_train_fused): raw split weights + occ_out in the eval
// image layout, then k_nof_eval_h3<true> with one BatchNorm coefficient set per chunk
size_t train_query_image_floats() { return EVAL_FLOATS; }

void pack_train_query(const NofParamsDev& P, float* img, hipStream_t s) {
  hipLaunchKernelGGL(k_pack_eval_vectors<true>, dim3(1), dim3(256), 0, s, P, img);   // occ_out, raw biases
  hipLaunchKernelGGL(k_eval_wscale<true>, dim3(8), dim3(1024), 0, s, P, img);
  hipLaunchKernelGGL(k_pack_eval_h3<true>, dim3((unsigned)((EH_VECS + 255) / 256)),
                     dim3(256), 0, s, P, img);
}

void launch_train_query(const float* rays, int stride, const float* z, int64_t total, int S, const float* ein,
                        const float* img, const float* coef, int64_t chunk, float* p_out, hipStream_t s,
                        float* hst, int64_t hst_chunk, int64_t hst_layer, int64_t store_chunks, const float* pts) {
  const int64_t C = (total + chunk - 1) / chunk;
  if (pts && hst) throw std::runtime_error("train query: no activation store with the point source");
  const int64_t ns = 16 * EH3_SB;
  const int64_t per = (std::min(chunk, total) + ns - 1) / ns;
  if (C >= 65536 || per >= ((int64_t)1 << 31)) throw std::runtime_error("train query: too many chunks / samples");
  // the stored chunks [0, Cs) and the rest as two launches: the store is compile-time in the kernel (a runtime
  // branch around the stores made every layer's first weight-ring wait drain them)
  const int64_t Cs = hst ? std::min(store_chunks, C) : 0;
  if (Cs > 0 && hst_layer * sizeof(float) > 0xffffffffull) throw std::runtime_error("train query: store layer >= 4 GiB");
  if (Cs > 0)
    hipLaunchKernelGGL((k_nof_eval_h3<true, true>), dim3((unsigned)per, (unsigned)Cs), dim3(256), 0, s, rays,
                       stride, z, total, S, ein, img, p_out, coef, chunk, hst, hst_chunk, hst_layer, 0);
  if (pts)
    launch_h3<true, true>(g_query_geometry < 0 ? EH3_GEOM_TRAIN : g_query_geometry, std::min(chunk, total),
                          (unsigned)C, s, pts, 3, (const float*)nullptr, total, 1, (const float*)nullptr, img, p_out,
                          coef, chunk, (float*)nullptr, (int64_t)0, (int64_t)0, 0);
  else if (C > Cs)
    launch_h3<true, false>(g_query_geometry < 0 ? EH3_GEOM_TRAIN : g_query_geometry, std::min(chunk, total),
                           (unsigned)(C - Cs), s, rays, stride, z, total, S, ein, img, p_out, coef, chunk,
                           (float*)nullptr, (int64_t)0, (int64_t)0, (int)Cs);
}

void launch_fold_logits(const float* rays, int stride, const float* z, int64_t total, int S, const float* ein,
                        const double* fold, int64_t chunk, float* p_out, hipStream_t s) {
  const int64_t blocks = (total + 255) / 256;
  if (blocks >= (int64_t)1 << 31) throw std::runtime_error("fold query: too many samples for one launch");
  const int64_t nfold = (total + chunk - 1) / chunk;
  if (nfold <= 1)
    hipLaunchKernelGGL(k_nof_eval_fold<0>, dim3((unsigned)blocks), dim3(256), 0, s, rays, stride, z, total, S, ein,
                       fold, total, (int64_t)1, p_out);
  else if (chunk >= 256)
    hipLaunchKernelGGL(k_nof_eval_fold<1>, dim3((unsigned)blocks), dim3(256), 0, s, rays, stride, z, total, S, ein,
                       fold, chunk, nfold, p_out);
  else
    hipLaunchKernelGGL(k_nof_eval_fold<2>, dim3((unsigned)blocks), dim3(256), 0, s, rays, stride, z, total, S, ein,
                       fold, chunk, nfold, p_out);
}

}  // namespace pcn

using namespace pcn;

extern "C" int pcnerf_nof_fold_eval(const pcnerf_nof_params* params, double* fold, void* stream) {
  PCN_API_BEGIN
  PCN_CHECK(params && fold, "pcnerf_nof_fold_eval: null argument");
  NofParamsDev P;
  PCN_CHECK(to_dev_params(params, 1e-5f, &P), "pcnerf_nof_fold_eval: null parameter pointer");
  hipLaunchKernelGGL(k_fold_eval, dim3(1), dim3(1024), 0, (hipStream_t)stream, P, fold);
  PCN_LAUNCH_CHECK("pcnerf_nof_fold_eval");
  PCN_API_END
}

extern "C" int pcnerf_nof_query_eval_fold(const float* rays, int64_t n_rays, int ray_stride, const float* z,
                                          int n_samples, const double* fold, float* p_out, void* stream) {
  PCN_API_BEGIN
  PCN_CHECK(rays && z && fold && p_out, "pcnerf_nof_query_eval_fold: null argument");
  PCN_CHECK(n_rays > 0 && n_samples > 0, "pcnerf_nof_query_eval_fold: empty input");
  PCN_CHECK(ray_stride >= 6, "pcnerf_nof_query_eval_fold: ray_stride < 6");
  const int64_t total = n_rays * (int64_t)n_samples;
  const int64_t blocks = (total + 255) / 256;
  PCN_CHECK(blocks < (int64_t)1 << 31, "pcnerf_nof_query_eval_fold: too many samples for one launch");
  {
    // algorithmic work per sample: 63 FMA + the encoding; bytes: z in, p out, ray rows
    ProfScope ps((hipStream_t)stream, PT_EVAL_FOLD, 126.0 * (double)total,
                 8.0 * (double)total + 4.0 * ray_stride * (double)n_rays);
    launch_fold_logits(rays, ray_stride, z, total, n_samples, nullptr, fold, total, p_out, (hipStream_t)stream);
  }
  PCN_LAUNCH_CHECK("pcnerf_nof_query_eval_fold");
  PCN_API_END
}

extern "C" int pcnerf_nof_forward_eval_fold(const float* emb, int64_t n, const double* fold, float* p_out,
                                            void* stream) {
  PCN_API_BEGIN
  PCN_CHECK(emb && fold && p_out, "pcnerf_nof_forward_eval_fold: null argument");
  PCN_CHECK(n > 0, "pcnerf_nof_forward_eval_fold: empty input");
  const int64_t blocks = (n + 255) / 256;
  PCN_CHECK(blocks < (int64_t)1 << 31, "pcnerf_nof_forward_eval_fold: too many samples for one launch");
  launch_fold_logits(nullptr, 0, nullptr, n, 1, emb, fold, n, p_out, (hipStream_t)stream);
  PCN_LAUNCH_CHECK("pcnerf_nof_forward_eval_fold");
  PCN_API_END
}

extern "C" int pcnerf_embed(const float* pts, int64_t n, float* out, void* stream) {
  PCN_API_BEGIN
  PCN_CHECK(pts && out, "pcnerf_embed: null argument");
  PCN_CHECK(n > 0, "pcnerf_embed: empty input");
  hipLaunchKernelGGL(k_embed, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, pts, n, out);
  PCN_LAUNCH_CHECK("pcnerf_embed");
  PCN_API_END
}

extern "C" size_t pcnerf_nof_eval_packed_floats(void) { return EVAL_FLOATS; }

extern "C" int pcnerf_nof_pack_eval(const pcnerf_nof_params* params, float* packed, void* stream) {
  PCN_API_BEGIN
  PCN_CHECK(params && packed, "pcnerf_nof_pack_eval: null argument");
  NofParamsDev P;
  PCN_CHECK(to_dev_params(params, 1e-5f, &P), "pcnerf_nof_pack_eval: null parameter pointer");
  hipStream_t s = (hipStream_t)stream;
  const unsigned nb = (unsigned)((OFF_BIAS + 255) / 256);
  hipLaunchKernelGGL(k_pack_eval_weights, dim3(nb), dim3(256), 0, s, P, packed);
  hipLaunchKernelGGL(k_pack_eval_vectors<false>, dim3(1), dim3(256), 0, s, P, packed);
  hipLaunchKernelGGL(k_eval_wscale<false>, dim3(8), dim3(1024), 0, s, P, packed);
  hipLaunchKernelGGL(k_pack_eval_h3<false>, dim3((unsigned)((EH_VECS + 255) / 256)),
                     dim3(256), 0, s, P, packed);
  PCN_LAUNCH_CHECK("pcnerf_nof_pack_eval");
  PCN_API_END
}

extern "C" int pcnerf_nof_query_eval(const float* rays, int64_t n_rays, int ray_stride, const float* z,
                                     int n_samples, const float* packed, float* p_out, void* stream) {
  PCN_API_BEGIN
  PCN_CHECK(rays && z && packed && p_out, "pcnerf_nof_query_eval: null argument");
  PCN_CHECK(n_rays > 0 && n_samples > 0, "pcnerf_nof_query_eval: empty input");
  PCN_CHECK(ray_stride >= 6, "pcnerf_nof_query_eval: ray_stride < 6");
  const int64_t total = n_rays * (int64_t)n_samples;
  const int64_t tiles = (total + 31) / 32;
  const int64_t blocks = (tiles + 3) / 4;
  PCN_CHECK(blocks < (int64_t)1 << 31, "pcnerf_nof_query_eval: too many samples for one launch");
  {
    // algorithmic work: 982,528 FLOP per sample (9 Linear layers); bytes: z in, p out, ray rows, network image
    ProfScope ps((hipStream_t)stream, PT_EVAL_QUERY, 982528.0 * (double)total,
                 8.0 * (double)total + 4.0 * ray_stride * (double)n_rays + 4.0 * EVAL_F32_FLOATS);
    launch_eval(rays, ray_stride, z, total, n_samples, nullptr, packed, p_out, (hipStream_t)stream);
  }
  PCN_LAUNCH_CHECK("pcnerf_nof_query_eval");
  PCN_API_END
}

extern "C" int pcnerf_nof_points_eval(const float* pts, int64_t n, const float* packed, float* p_out, void* stream) {
  PCN_API_BEGIN
  PCN_CHECK(pts && packed && p_out, "pcnerf_nof_points_eval: null argument");
  PCN_CHECK(n > 0, "pcnerf_nof_points_eval: empty input");
  const int64_t blocks = ((n + 31) / 32 + 3) / 4;
  PCN_CHECK(blocks < (int64_t)1 << 31, "pcnerf_nof_points_eval: too many samples for one launch");
  PCN_CHECK(g_eval_math == 1, "pcnerf_nof_points_eval: needs eval math 1 (split fp16); under eval math 0 embed the "
                              "points (pcnerf_embed) and call pcnerf_nof_forward_eval");
  {
    // algorithmic work: 982,528 FLOP per sample; bytes: the position in, p out, network image
    ProfScope ps((hipStream_t)stream, PT_EVAL_QUERY, 982528.0 * (double)n, 16.0 * (double)n + 4.0 * EVAL_F32_FLOATS);
    launch_eval(nullptr, 0, nullptr, n, 1, nullptr, packed, p_out, (hipStream_t)stream, pts);
  }
  PCN_LAUNCH_CHECK("pcnerf_nof_points_eval");
  PCN_API_END
}

extern "C" int pcnerf_nof_forward_eval(const float* emb, int64_t n, const float* packed, float* p_out,
                                       void* stream) {
  PCN_API_BEGIN
  PCN_CHECK(emb && packed && p_out, "pcnerf_nof_forward_eval: null argument");
  PCN_CHECK(n > 0, "pcnerf_nof_forward_eval: empty input");
  const int64_t blocks = ((n + 31) / 32 + 3) / 4;
  PCN_CHECK(blocks < (int64_t)1 << 31, "pcnerf_nof_forward_eval: too many samples for one launch");
  launch_eval(nullptr, 0, nullptr, n, 1, emb, packed, p_out, (hipStream_t)stream);
  PCN_LAUNCH_CHECK("pcnerf_nof_forward_eval");
  PCN_API_END
}


extern "C" int pcnerf_set_query_geometry(int geometry) {
  if (geometry < -1 || geometry > 3) {
    pcn::set_error("pcnerf_set_query_geometry: geometry must be -1 (default) or 0..3 (bit 0: 8-wave workgroup, "
                   "bit 1: 4-slot weight ring)");
    return -2;
  }
  const int prev = pcn::g_query_geometry;
  pcn::g_query_geometry = geometry;
  return prev;
}

extern "C" int pcnerf_set_train_query_form(int form) {
  if (form != -1 && form != 0 && form != 2 && form != 4) {
    pcn::set_error("pcnerf_set_train_query_form: train_query_form must be -1 (default), 0 (6 sample blocks), 2 "
                   "(7 sample blocks) or 4 (8 sample blocks); 1 (half-skewed) and 3 are not built");
    return -2;
  }
  const int prev = pcn::g_train_query_form;
  pcn::g_train_query_form = form;
  return prev;
}

extern "C" int pcnerf_set_eval_math(int mode) {
  if (mode < 0 || mode > 1) {
    pcn::set_error("pcnerf_set_eval_math: mode must be 0 (fp32 MFMA) or 1 (split fp16, 3 products)");
    return -1;
  }
  const int prev = pcn::g_eval_math;
  pcn::g_eval_math = mode;
  return prev;
}
