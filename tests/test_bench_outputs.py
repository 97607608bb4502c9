"""bench.py as a caller sees it: a plain run times exactly --steps sample-steps and prints one line without the --full
sections; --dump-outputs writes what the last timed step computed, and two runs with the same arguments write the same
arrays (seeded inputs, bit-reproducible step)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

ARGS = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--nsamples", "4"]


def _run(out_dir):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + ARGS + ["--dump-outputs", str(out_dir)],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:]
    return lines[0], {f[:-len(".npy")]: np.load(os.path.join(out_dir, f)) for f in sorted(os.listdir(out_dir))}


def test_dump_outputs_samples_large_arrays_the_same_way(tmp_path):
    import torch
    from types import SimpleNamespace
    import bench
    big = torch.arange(3 * bench.DUMP_MAX_ELEMS + 5, dtype=torch.float32).reshape(-1, 1)     # a grouped LWC bound's shape
    small = torch.linspace(-1, 1, 12).reshape(4, 3)
    runner = SimpleNamespace(loss=torch.tensor([2.5]))
    opt = SimpleNamespace(norm=torch.tensor([0.75, 0.0]), named=[("up", big), ("scale", small)])
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), runner, opt)
    a = {f: np.load(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")}
    assert sorted(a) == ["grad_norm.npy", "loss.npy", "param.scale.npy", "param.up.npy"]
    assert a["loss.npy"].tolist() == [2.5] and a["grad_norm.npy"].tolist() == [0.75]
    assert np.array_equal(a["param.scale.npy"], small.numpy())
    s = a["param.up.npy"]
    assert s.dtype == np.float32 and s.shape == (bench.DUMP_MAX_ELEMS,)
    assert (np.diff(s) > 0).all() and s[0] >= 0 and s[-1] < big.numel()        # distinct elements, in index order
    assert np.array_equal(s, np.load(tmp_path / "b" / "param.up.npy"))
    too_big = [("w%d" % i, torch.zeros(bench.DUMP_MAX_ELEMS)) for i in range(17)]
    with pytest.raises(SystemExit):
        bench.dump_outputs(str(tmp_path / "c"), runner, SimpleNamespace(norm=opt.norm, named=too_big))


@pytest.mark.gpu
def test_plain_bench_line_and_dumped_outputs(tmp_path):
    line, out = _run(tmp_path / "a")
    assert (line["metric"], line["unit"], line["higher_is_better"], line["dtype"]) == \
        ("calibration_sample_steps_per_sec", "sample-steps/s", True, "bf16")
    assert (line["steps"], line["warmup"], line["n_gpus"]) == (3, 1, 1)
    assert line["ms_per_step"] > 0 and line["value"] * line["ms_per_step"] == pytest.approx(1e3, rel=1e-9)
    assert not {"roofline", "roofline_int8", "roofline_hbm", "end_to_end", "cpu_baseline"} & set(line)
    assert {"loss", "grad_norm"} <= set(out) and any(k.startswith("param.") for k in out)
    assert all(a.dtype == np.float32 and a.size and np.isfinite(a).all() for a in out.values())
    assert sum(a.nbytes for a in out.values()) <= 64 << 20
    assert float(out["loss"][0]) == line["config"]["last_loss"]
    _, again = _run(tmp_path / "b")
    assert sorted(again) == sorted(out)
    for k in out:
        assert np.array_equal(again[k], out[k]), k
