"""bench.py's plain run on the GPU, in this process: the line's keys, --steps, and --dump-outputs."""
import importlib.util
import json
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(HERE, "..", "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _run(bench, capsys, out, steps):
    bench.main(["--gpus", "1", "--steps", str(steps), "--warmup", "1", "--rays", "1000", "--samples", "32",
                "--importance", "64", "--dump-outputs", str(out)])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    return line, {f[:-4]: np.load(os.path.join(out, f)) for f in sorted(os.listdir(out)) if f.endswith(".npy")}


@pytest.fixture
def rng_restored():
    """bench.py seeds torch's generators; the tests after this one find them as they were."""
    import torch
    cpu, gpu = torch.get_rng_state(), torch.cuda.get_rng_state()
    yield
    torch.set_rng_state(cpu)
    torch.cuda.set_rng_state(gpu)


def test_plain_run_line_and_dumped_outputs(bench, tmp_path, capsys, rng_restored):
    """A plain run (1,000 rays, no multiple of a tile) prints the contract's keys with the CPU legs null, times
    exactly --steps steps, and writes the last timed step's result dict and loss.  A second run with the same
    arguments draws the same perturbations: its outputs agree to the bound smoke() holds against the oracle (rtol
    1e-4; the runs differ only by the order of the kernels' atomic float64 sums), while a run one step longer ends
    on other draws."""
    line, a = _run(bench, capsys, tmp_path / "a", 2)
    for k in bench.REQUIRED_KEYS:
        assert k in line, k
    assert line["steps"] == 2 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["value"] > 0
    assert line["value"] == pytest.approx(1000 / (1e-3 * line["ms_per_step"]), rel=1e-2)
    assert line["cpu_baseline"] is None and line["cd_vs_ref"] is None and "extras" not in line
    assert line["roofline"]["kernel"] and "detail" not in line
    assert set(a) == {"depth", "depth_fine", "child_free_loss", "child_depth_loss", "child_free_loss_fine",
                      "child_depth_loss_fine", "loss"}
    assert a["depth_fine"].shape == (1000,) and a["depth_fine"].dtype == np.float32
    assert float(a["loss"]) == pytest.approx(line["loss"], rel=1e-6)
    _, b = _run(bench, capsys, tmp_path / "b", 2)
    for k in a:
        assert np.isfinite(a[k]).all(), k
        np.testing.assert_allclose(b[k], a[k], rtol=1e-4, atol=1e-9, err_msg=k)
    _, c = _run(bench, capsys, tmp_path / "c", 3)
    assert np.abs(c["depth"] - a["depth"]).max() > 1e-4 * np.abs(a["depth"]).max()
