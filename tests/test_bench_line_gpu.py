"""bench.py's line on the GPU, end to end.  --full: one subprocess run with few steps, every object the contract and DESIGN.md section 5 name is
there and NO extra leg failed (an extra's exception is caught into {"error": ...} so that it never costs the headline -- which also means nothing
else notices it: round 5 shipped a NameError in all four legs for an hour)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_default_line_has_every_object_and_no_failed_leg():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--steps", "4", "--warmup", "2", "--long-steps", "8", "--cpu-steps", "1"],
                       capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
    d = json.loads(line)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config",
              "roofline", "cpu_baseline", "long_run", "parity", "extra"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 4 and d["warmup"] == 2 and d["dtype"] == "f32" and d["vs_baseline"] is None and "workload" in d["config"]
    rf = d["roofline"]
    assert rf["bound"] == "hbm" and rf["unit"] == "GB/s" and rf["peak"] == 8000.0 and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-12
    assert rf["kernel"] in rf["all_kernels"] and rf["kernel"] == max(rf["dominant_by"]["ms_per_step"], key=rf["dominant_by"]["ms_per_step"].get)
    assert "traffic" in rf and (rf["traffic"] is not None or "traffic_unavailable" in rf)
    m = rf["mfma"]
    assert m["peak"] == 157.3 and 0.1 < m["frac"] < 1.0 and abs(m["frac"] - m["achieved_tflops"] / m["peak"]) < 1e-12 and m["flop_per_launch"] == 2 * 4096 * 48 * 22912
    cb = d["cpu_baseline"]
    assert cb["kind"] == "port" and cb["cores"] >= 1 and cb["value"] > 0 and "sample" in cb
    p = d["parity"]
    assert "error" not in p and p["max_abs_rgb"] <= 1e-3 and p["max_abs_thermal"] <= 1e-3, p
    assert 0 < p["density_err_over_1ulp_response"] <= 6.0 and 0 <= p["bins_beyond_64ulp_share"] <= 0.02, p
    for name, leg in d["extra"].items():
        assert "error" not in leg, (name, leg)
        if name == "eval_render":  # the reference's TEST_RAYS_PER_SEC: full images through the Model API and through tn_render_rays_eval
            for k in ("get_outputs_for_camera", "tn_render_rays_eval"):
                assert leg[k]["ms"] > 0 and leg[k]["rays_per_s"] > 1e6 and 0 < leg[k]["frac_of_hbm_roofline"] < 1.0, (name, leg)
            assert leg["rays"] == 640 * 480 + 160 * 120
            continue
        assert leg["ms_per_step"] > 0 and leg["rays_per_s"] > 0, (name, leg)
        if name == "head_bf16x3":  # the opt-in split-bf16 colour head: its own dtype, its own parity block, the fp32 step of the same run beside it
            assert "bf16x3" in leg["dtype"] and leg["f32_same_run"]["ms_per_step"] > 0
            assert leg["parity"]["max_abs_rgb"] <= 1e-3 and leg["parity"]["max_abs_thermal"] <= 1e-3, leg
            assert 0 < leg["gradients_vs_f32_path"]["head_max"] <= 3e-3, leg  # (3e-4 without a flipped ReLU mask; measured 3e-5)
    assert set(d["extra"]) == {"separate_8192", "nerf_samples_96", "model_api_amp", "fused_trainer", "eval_render", "head_bf16x3"}
    ak = rf["all_kernels"]
    assert all(v["bound"] == ("l2" if k.startswith("k_prop_fwd") else "hbm") and 0 < v["frac"] < 1.0 for k, v in ak.items()), ak


def test_plain_line_is_the_headline_and_its_dump_is_the_same_every_run(tmp_path):
    """Without --full: the headline keys only and --steps timed steps.  --dump-outputs: the second step of the timed path replayed from a fixed
    state -- its losses, the parameters it started from and the Adam moments it left (float32 / float64, under 64 MB) -- the same in two runs up
    to rounding: each array within 1e-3 of its own largest magnitude (measured: 2.4e-4 on the camera poses, whose gradient is a cancelling sum
    over every ray; 1e-6 and below elsewhere), the losses within 1e-5."""
    import numpy as np

    dumps = []
    for run in ("a", "b"):
        out = tmp_path / run
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(out)],
                           capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-2000:]
        d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
        assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["unit"] == "rays/s" and d["higher_is_better"] is True
        assert abs(d["value"] - 4096 * 1e3 / d["ms_per_step"]) <= 1e-6 * d["value"]
        for k in ("roofline", "long_run", "parity", "extra", "cpu_baseline"):
            assert k not in d, k
        files = sorted(out.glob("*.npy"))
        assert sum(f.stat().st_size for f in files) <= 64 << 20
        dumps.append({f.name[:-len(".npy")]: np.load(f) for f in files})
    a, b = dumps
    assert a.keys() == b.keys()
    assert {n.split(".")[0] for n in a} == {"loss", "param_in", "exp_avg", "exp_avg_sq"}
    table = "field.mlp_base.model.0.hash_table"
    assert np.abs(a[f"exp_avg.{table}"]).max() > 0 and np.abs(a[f"exp_avg_sq.{table}"]).max() > 0  # the backward's magnitudes are in the dump
    for name in a:
        assert a[name].dtype in (np.float32, np.float64) and np.isfinite(a[name]).all(), name
        x, y = a[name].astype(np.float64), b[name].astype(np.float64)
        if name.startswith("loss."):
            assert np.allclose(x, y, rtol=1e-5, atol=0), (name, x, y)
        else:
            assert np.abs(x - y).max() <= 1e-3 * np.abs(x).max(), (name, float(np.abs(x - y).max()), float(np.abs(x).max()))
