"""Small files in the reference's own on-disk formats for tests/test_io_metrics.py, under tests/golden/io_files/:
the head (first HEAD points, header counts rewritten, payload bytes as stored) of three binary PCDs of the
reference's checkout -- frame 1153's source cloud and its version_1 two-step render, KITTI-00 scan 1151 --, the
frame's one-point pose PCD as it is, and the first whole ray groups (at most HEAD rows) of frame 1153's two-step side
file other_interest_sub_nerf_number_child.npy.

usage: python make_io_files.py <root of the reference checkout>"""
import os
import re
import shutil
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "io_files")
HEAD = 4096
RENDER = "logs/kitti00/1151_1200_view/render_result"
SIDE = "logs/kitti00/1151_1200_view/two_step/1153pcd/childnerf_ray_intersect"


def pcd_head(src, dst, n=HEAD):
    """The first ``n`` points of a binary xyz float32 PCD: the header's own lines with WIDTH / POINTS set to ``n``."""
    b = open(src, "rb").read()
    i = b.index(b"DATA binary\n") + len(b"DATA binary\n")
    head = re.sub(rb"(?m)^(WIDTH|POINTS) \d+$", lambda m: m.group(1) + b" %d" % n, b[:i])
    assert len(b) - i >= 12 * n
    with open(dst, "wb") as fh:
        fh.write(head + b[i:i + 12 * n])


def main(ref):
    os.makedirs(OUT, exist_ok=True)
    pcd_head(os.path.join(ref, RENDER, "source/1153_source.pcd"), os.path.join(OUT, "1153_source.pcd"))
    pcd_head(os.path.join(ref, RENDER, "infer/version_1_1153_two_step.pcd"),
             os.path.join(OUT, "version_1_1153_two_step.pcd"))
    shutil.copyfile(os.path.join(ref, RENDER, "source/1153_pose.pcd"), os.path.join(OUT, "1153_pose.pcd"))
    pcd_head(os.path.join(ref, "data/kitti/00/pcd_remove_dynamic/1151.pcd"), os.path.join(OUT, "1151.pcd"))
    other = np.load(os.path.join(ref, SIDE, "other_interest_sub_nerf_number_child.npy"), allow_pickle=False)
    i = 0
    while i + int(other.reshape(-1)[i]) + 1 <= HEAD:   # whole groups: the first row of a group holds its size - 1
        i += int(other.reshape(-1)[i]) + 1
    np.save(os.path.join(OUT, "other_interest_sub_nerf_number_child.npy"), other[:i])


if __name__ == "__main__":
    main(sys.argv[1])
