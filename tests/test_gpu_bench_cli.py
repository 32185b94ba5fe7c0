"""bench.py's plain run and --dump-outputs, end to end in a fresh child process: the plain line times exactly --steps steps and
carries the contract's keys and nothing of the --full record; the dump holds what the last timed step computed, float32 / float64,
within 64 MB, and two runs with the same arguments write the same arrays (a dump run forms its sums in a fixed order)."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "n_gpus", "steps", "warmup")


def _bench(args, tmp_path, timeout=600):
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "NERAF_DETERMINISTIC"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, cwd=str(tmp_path), stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=timeout)
    assert p.returncode == 0, (p.stdout.decode(errors="replace")[-2000:], p.stderr.decode(errors="replace")[-4000:])
    lines = [ln for ln in p.stdout.decode().splitlines() if ln.startswith("{")]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


def _dumped(d):
    files = sorted(glob.glob(os.path.join(d, "*.npy")))
    arrays = {os.path.basename(f)[:-4]: np.load(f) for f in files}
    assert arrays and sum(os.path.getsize(f) for f in files) <= 64 << 20
    for k, v in arrays.items():
        assert v.dtype in (np.float32, np.float64), (k, v.dtype)
        assert np.isfinite(v).all(), k
    return arrays


def test_plain_train_line_and_dump(tmp_path):
    out = tmp_path / "dump"
    d = _bench(["--gpus", "1", "--steps", "3", "--warmup", "1", "--rays", "1024", "--slices", "256", "--dump-outputs", str(out)], tmp_path)
    for k in KEYS:
        assert k in d, k
    assert d["steps"] == 3 and d["warmup"] == 1 and d["higher_is_better"] is True and d["dtype"] == "f16"
    assert abs(d["value"] - (1024 + 256 * 513) / (d["ms_per_step"] * 1e-3)) <= 1e-3 * d["value"]
    for k in ("roofline", "cpu_baseline", "eval_render", "parity", "hip_graphs"):
        assert k not in d, k
    assert d["detail"] is None and d["config"]["deterministic"] is True
    a = _dumped(str(out))
    assert a["loss"].shape == () and "loss_dict.rgb_loss" in a and "loss_dict.audio_sc_loss" in a
    assert any(k.startswith("param.audio.resnet3d") for k in a) and any(k.startswith("grad.vision.") for k in a)
    # the summed loss is the loss dict's sum (train_iteration's return values of the same step)
    parts = sum(float(v) for k, v in a.items() if k.startswith("loss_dict."))
    assert abs(float(a["loss"]) - parts) <= 1e-4 * abs(parts) + 1e-7


def test_plain_eval_line_and_dump(tmp_path):
    out = tmp_path / "dump"
    d = _bench(["--mode", "eval", "--steps", "1", "--warmup", "1", "--rirs", "2", "--dump-outputs", str(out)], tmp_path)
    for k in KEYS:
        assert k in d, k
    assert d["steps"] == 1 and d["mode"] == "eval" and "roofline" not in d and "cpu_baseline" not in d
    a = _dumped(str(out))
    assert a["frame.rgb"].size == min(684 * 1024 * 3, 1 << 18)      # above the per-array cap: a seeded sample
    assert a["rir.raw_output"].shape == (2, 60, 1, 513)


def test_two_dump_runs_write_the_same_arrays(tmp_path):
    """The default mode's fp32 atomics make two runs of the chaotic encoder part by far more than rounding after the priming steps;
    a --dump-outputs run sums in a fixed order (NERAF_DETERMINISTIC=1, set by bench.py), so the same arguments give the same
    outputs.  The radiance loss VALUES are still summed atomically (reported only, they feed nothing back): rounding, hence rtol."""
    args = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--rays", "1024", "--slices", "256"]
    _bench(args + ["--dump-outputs", str(tmp_path / "a")], tmp_path)
    _bench(args + ["--dump-outputs", str(tmp_path / "b")], tmp_path)
    a, b = _dumped(str(tmp_path / "a")), _dumped(str(tmp_path / "b"))
    assert a.keys() == b.keys()
    same = sum(np.array_equal(a[k], b[k]) for k in a)
    print(f"{same} of {len(a)} arrays bit-identical")
    for k in a:
        np.testing.assert_allclose(b[k], a[k], rtol=1e-5, atol=1e-7 * float(np.abs(a[k]).max()), err_msg=k)
