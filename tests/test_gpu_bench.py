"""bench.py end to end on the GPU at a 64-clip batch: a plain run times --steps steps of
the headline alone and --dump-outputs writes the last step's logits (the same from run
to run, and what a direct forward of the bench's model on the bench's input returns);
--full adds the parity sample, the other precision modes and the CPU baseline."""
import json

import numpy as np
import pytest
import torch

import bench

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
B = 64
EXTRA = ("parity", "cpu_baseline", "bf16x3_mode", "f32_mode", "bf16_mode", "c2_cnn_trad_pool2", "c3_res8_bf16",
         "c5_res26_narrow_train")


def _line(capsys, argv):
    capsys.readouterr()
    bench.main(argv)
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


def test_plain_run_is_the_headline_alone_and_dumps_its_logits(capsys, tmp_path):
    argv = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", str(B)]
    d = _line(capsys, argv + ["--dump-outputs", str(tmp_path / "a")])
    assert d["metric"] == bench.METRIC and d["unit"] == "clips/s" and d["higher_is_better"] is True
    assert d["dtype"] == "f16x2" and d["steps"] == 3 and d["warmup"] == 1
    assert d["ms_per_step"] > 0
    # value = clips of the timed steps over their time; ms_per_step the same time per step
    assert abs(d["value"] * d["ms_per_step"] * 1e-3 / B - 1) < 1e-2
    assert not [k for k in EXTRA if k in d] and "fixtures" not in d["f16x2_admission"]
    a = np.load(tmp_path / "a" / "logits.npy")
    assert a.dtype == np.float32 and a.shape == (B, 12) and np.isfinite(a).all()
    _line(capsys, argv + ["--dump-outputs", str(tmp_path / "b")])
    assert np.array_equal(a, np.load(tmp_path / "b" / "logits.npy"))
    m = bench.bench_model("res15", torch.device(DEV))
    x = bench.mfcc_like(B, DEV, torch.Generator(device=DEV).manual_seed(1234))
    with torch.no_grad():
        assert np.array_equal(a, m(x).cpu().numpy())


def test_full_run_adds_parity_fixtures_and_cpu_baseline(capsys):
    d = _line(capsys, ["--steps", "1", "--warmup", "1", "--batch", "8", "--full", "--no-alt", "--cpu-seconds", "0.1"])
    assert d["dtype"] == "f16x2" and d["parity"]["max_abs_logit_err_vs_oracle_f64"] <= 1e-4
    assert d["parity"]["sample_clips"] == 8 and d["cpu_baseline"]["value"] > 0
    assert "error" not in d["f16x2_admission"]["fixtures"]
    assert set(d["modes"]) == {"res15_f16x2 (headline)", "cpu_baseline"}


def test_full_run_adds_the_other_modes(capsys):
    d = _line(capsys, ["--steps", "1", "--warmup", "1", "--batch", "8", "--full", "--no-configs", "--no-cpu-baseline"])
    for k, bar in (("bf16x3_mode", 1e-4), ("f32_mode", 1e-4), ("bf16_mode", None)):
        assert d[k]["value"] > 0 and d[k]["ms_per_step"] > 0
        assert bar is None or d[k]["parity"]["max_abs_logit_err_vs_oracle_f64"] <= bar
    assert set(d["modes"]) == {"res15_f16x2 (headline)", "res15_bf16x3", "res15_f32", "res15_bf16"}
