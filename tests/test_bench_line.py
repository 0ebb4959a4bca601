"""bench.py's stdout contract (CPU): ONE compact JSON line that the driver's 8 KB tail holds completely, with every BASELINE row in it;
the plain run (headline only) and --dump-outputs, on the CPU and (marked gpu) end to end."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _verbose_record():
    # a full record of an earlier run (what `bench.py --full --verbose` prints and what its --verbose-out file holds)
    for line in open(os.path.join(ROOT, "profiles", "r04_bench_cfg2.json")):
        if line.startswith("{"):
            return json.loads(line)
    raise AssertionError("no record")


def test_compact_line_fits_the_drivers_tail_and_names_every_baseline_row():
    import bench

    rec = _verbose_record()
    line = bench.compact_line(rec, os.path.join(ROOT, "gpurun_out", "bench_verbose_cfg2_n1.json"))
    text = json.dumps(line)
    assert len(text) <= 4096, len(text)
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
                "data", "config", "roofline", "cpu_baseline"):
        assert key in line, key
    assert line["config"]["workload"].startswith("cfg2") and "model" not in line["config"]
    r = line["roofline"]
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3 and "traffic" in r
    assert abs(r["achieved"] - r["algorithmic_bytes"] / (line["ms_per_step"] * 1e-3) / 1e9) < 2.0  # B / t, GB/s
    for key in ("value", "unit", "cores", "kind", "sample"):
        assert key in line["cpu_baseline"], key
    # the BASELINE configurations (configs[2..4], cfg5 both as a shard and as stated) and the out-of-cache workload
    for row in ("cfg3", "cfg4", "cfg5", "cfg5_strong", "hbm", "cfg3_rough", "cfg5_rough", "cfg2_theta150", "cfg2_batch8"):
        e = line["configs"][row]
        assert e["us"] > 0 and 0 < e["frac"] < 1 and "dom_us" in e and "prep_ms" in e, row
        assert abs(e["us"] - rec["also"][row]["ms_per_step"] * 1e3) <= 1e-3 * e["us"]
    assert line["verbose"] == "gpurun_out/bench_verbose_cfg2_n1.json"


def test_comm_model_matches_the_design_table():
    """cfg5's C1 (3.7 MB) at N = 2 / 4 / 8 = 12 + 37, 18 + 18.5, 25 + 9.3 us; C2 twice the bytes."""
    import bench

    c1 = 720 * 1280 * 4
    assert abs(bench.comm_model_us(c1, 2) - (12 + 36.9)) < 0.2
    assert abs(bench.comm_model_us(c1, 4) - (18 + 18.4)) < 0.2
    assert abs(bench.comm_model_us(c1, 8) - (25 + 9.2)) < 0.2
    assert abs(bench.comm_model_us(2 * c1, 8) - (25 + 18.4)) < 0.2
    assert abs(bench.comm_model_us(16, 8) - 25.0) < 0.01


def test_band_model_matches_the_design_table():
    """DESIGN.md section 5, row-band partition of cfg5 (1280 wide, 20 halo rows = 102 KB per exchange and direction = 1.0 us on the wire):
    two exchanges at 8 + 1 us, the statistics' all-reduce at alpha(N), the patch gradient's 4 KB at alpha(N) + its wire time."""
    import bench

    assert abs(bench.band_model_us(27.5, 1280, 8) - (27.5 + 2 * (8 + 1.024) + 25.0 + 25.0 + 0.01)) < 0.1
    assert abs(bench.band_model_us(48.0, 1280, 2) - (48.0 + 2 * (8 + 1.024) + 12.0 + 12.04)) < 0.1
    assert abs(bench.band_model_us(27.5, 1280, 8, patch_gradient=False) - (27.5 + 18.05 + 25.0)) < 0.1
    assert bench.band_model_us(85.0, 1280, 1) == 85.0


def test_plain_run_is_the_default_and_the_rest_sits_behind_full():
    """`bench.py --gpus 1 --steps K --warmup W` times exactly K steps (one window) and nothing else; --full brings back the rest."""
    import bench

    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "3"])
    assert (a.steps, a.warmup, a.windows, a.full, a.dump_outputs, a.verbose_out) == (7, 3, 1, False, None, None)
    b = bench.parse_args(["--full", "--dump-outputs", "out"])
    assert b.full and b.dump_outputs == "out"


def test_compact_line_of_a_plain_record():
    """A plain run's record has no per-kernel passes, other rows or CPU baselines: the line keeps the contract's keys and the
    evaluation's roofline, and names no full record when none was written."""
    import bench

    rec = _verbose_record()
    for k in ("also", "cpu_baseline", "cpu_baseline_torch", "graph_replay"):
        rec.pop(k, None)
    rec["roofline"] = {k: v for k, v in rec["roofline"].items() if k not in ("dominant", "kernels", "method")}
    line = bench.compact_line(rec, None)
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "dtype", "roofline", "loss"):
        assert key in line, key
    for key in ("configs", "cpu_baseline", "graph_replay_us", "verbose"):
        assert key not in line, key
    r = line["roofline"]
    assert "dominant" not in r and "kernels_us" not in r
    assert abs(r["achieved"] - r["algorithmic_bytes"] / (line["ms_per_step"] * 1e-3) / 1e9) < 2.0



def test_bench_compact_reads_a_plain_record(tmp_path):
    """tools/bench_compact.py (the A/B scripts' view) on a record without per-kernel passes, as a plain run writes it."""
    import subprocess

    rec = _verbose_record()
    rec.pop("also", None)
    rec["roofline"] = {k: v for k, v in rec["roofline"].items() if k not in ("dominant", "kernels", "method")}
    path = tmp_path / "plain.log"
    path.write_text(json.dumps(rec) + "\n")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bench_compact.py"), str(path), "[plain]"], capture_output=True, text=True,
                       timeout=60)
    assert p.returncode == 0, p.stderr[-2000:]
    assert p.stdout.startswith("[plain] cfg2:") and "kernels {}" in p.stdout

def test_dump_outputs_writes_float_arrays_within_the_limit(tmp_path):
    import numpy as np

    import bench

    names = bench.dump_outputs(str(tmp_path / "d"), {"result": np.arange(8, dtype=np.float64), "iwe": np.ones((3, 4), dtype=np.float16),
                                                     "grad": np.array([1, 2], dtype=np.int64)})
    assert names == ["grad.npy", "iwe.npy", "result.npy"]
    assert np.load(tmp_path / "d" / "result.npy").dtype == np.float64
    assert np.load(tmp_path / "d" / "iwe.npy").dtype == np.float32 and np.load(tmp_path / "d" / "grad.npy").dtype == np.float32
    with pytest.raises(ValueError):
        bench.dump_outputs(str(tmp_path / "e"), {"big": np.zeros(bench.DUMP_LIMIT_BYTES // 8 + 1, dtype=np.float64)})
    assert not (tmp_path / "e").exists()


def _plain_run(out_dir):
    import subprocess

    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "5", "--warmup", "2", "--ramp", "0",
           "--dump-outputs", str(out_dir)]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_bench_dumps_the_outputs_of_its_last_step(tmp_path):
    """Two plain runs with the same arguments, as separate processes: one line each, the headline alone, and the same outputs."""
    import numpy as np

    a, b = _plain_run(tmp_path / "a"), _plain_run(tmp_path / "b")
    for line in (a, b):
        assert line["steps"] == 5 and line["warmup"] == 2 and line["ms_per_step"] > 0 and line["value"] > 0
        assert line["unit"] == "events/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
        assert "configs" not in line and "cpu_baseline" not in line and "dominant" not in line["roofline"]
    out = {}
    for run in ("a", "b"):
        out[run] = {name: np.load(tmp_path / run / (name + ".npy")) for name in ("result", "grad", "iwe")}
        assert sorted(os.listdir(tmp_path / run)) == ["grad.npy", "iwe.npy", "result.npy"]
    ra, rb = out["a"], out["b"]
    assert ra["result"].shape == (8,) and ra["grad"].shape == (2,) and ra["iwe"].ndim == 2
    for name in ("result", "grad", "iwe"):
        assert np.isfinite(ra[name]).all()
        assert np.allclose(ra[name], rb[name], rtol=1e-5, atol=1e-6 * np.abs(ra[name]).max()), name


@pytest.mark.gpu
def test_plain_bench_times_exactly_k_steps_and_dumps_what_the_oracle_computes(tmp_path, monkeypatch, capsys):
    """bench.main in this process with every evaluation counted: W warm-up + K timed evaluations and nothing else (no ramp, no
    settle windows, no instrumented passes), ONE window of K, and the dumped result / gradient / image against the CPU oracle on
    bench.make_inputs' own events at the fp32 theta the prepared call reads (the plain 1e-4 gate of the full-size tests)."""
    import numpy as np

    import bench
    import event_based_optical_flow_amd as E
    from oracle import oracle as orc

    K, W = 37, 3
    calls = []
    prepare = E.CMaxHandle.prepare

    def counting_prepare(self, *a, **kw):
        call, res, grad = prepare(self, *a, **kw)

        def counted():
            calls.append(1)
            call()

        counted.motion = call.motion
        return counted, res, grad

    monkeypatch.setattr(E.CMaxHandle, "prepare", counting_prepare)
    vpath = tmp_path / "record.json"
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", str(K), "--warmup", str(W), "--ramp", "0", "--no-pin",
                                      "--dump-outputs", str(tmp_path / "d"), "--verbose-out", str(vpath)])
    bench.main()
    line = json.loads([l for l in capsys.readouterr().out.splitlines() if l.startswith("{")][-1])
    assert len(calls) == W + K
    rec = json.load(open(vpath))
    t = rec["timing"]
    assert t["windows"] == 1 and t["steps_per_window"] == K and line["steps"] == K
    assert abs(line["ms_per_step"] - t["median"]) <= 1e-5 * t["median"]

    cfg = bench.WORKLOADS["cfg2"]
    ev, motion, _ = bench.make_inputs(cfg, 0, 1)
    theta32 = np.asarray(motion, dtype=np.float32).astype(np.float64)
    ref = orc.objective(ev, theta32, "2d-translation", (cfg["H"], cfg["W"]), cost=cfg["cost"], sigma=cfg["sigma"])
    d = {name: np.load(tmp_path / "d" / (name + ".npy")) for name in ("result", "grad", "iwe")}
    assert abs(d["result"][0] - ref["loss"]) <= 1e-4 * abs(ref["loss"])
    assert np.abs(d["grad"] - ref["grad"]).max() <= 1e-4 * np.abs(ref["grad"]).max()
    assert np.abs(d["iwe"] - ref["iwes"]["iwe"]).max() <= 1e-4 * np.abs(ref["iwes"]["iwe"]).max()
