"""bench.py's output contract (CPU): the driver parses the LAST stdout line; it must be one strict-JSON record below 6 KB that carries
the headline with its `roofline` and `cpu_baseline` (round 4's single 20.85-KB line was not parsed: BENCH_r04.parsed = null)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _strict(line):
    def bad(tok):
        raise ValueError("non-finite token " + tok)
    return json.loads(line, parse_constant=bad)


def _check(line):
    assert "\n" not in line and len(line) < 6000, len(line)
    c = _strict(line)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config",
              "roofline", "cpu_baseline", "parity", "first_solve_ms", "repeat_identical"):
        assert k in c, k
    assert "workload" in c["config"] and "model" not in c["config"]
    for k in ("kernel", "bound", "achieved", "peak", "unit", "frac", "traffic", "algorithmic_bytes_per_launch", "avg_launch_us"):
        assert k in c["roofline"], k
    assert c["roofline"]["bound"] in ("hbm", "mfma") and c["roofline"]["unit"] in ("GB/s", "TFLOP/s")
    for k in ("value", "unit", "cores", "kind", "nproc", "cpu", "sample"):
        assert k in c["cpu_baseline"], k
    for k in ("ok", "dt_m", "dr_rad"):
        assert k in c["parity"], k
    for blk in ("secondary", "c4_1gpu", "online_c5", "batched"):
        assert blk in c and "value" in c[blk] or blk == "online_c5" and "wall_s" in c[blk], blk
    assert c["secondary"]["roofline"]["frac"] and c["secondary"]["cpu_baseline"]["value"]
    assert c["c4_1gpu"]["roofline"]["frac"] and c["c4_1gpu"]["cpu_baseline"]["value"] and "ms_per_solve" in c["c4_1gpu"]
    assert c["online_c5"]["roofline"]["frac"] and c["online_c5"]["cpu_baseline"]["value"]
    txt = json.dumps(c)
    assert '"note"' not in txt and "NaN" not in txt and "Infinity" not in txt
    return c


def test_compact_record_of_a_full_round4_record():
    import bench
    full = json.load(open(os.path.join(ROOT, "profiles", "bench_r04c.json")))
    assert len(json.dumps(full)) > 15000                      # the record that did not fit
    _check(bench.compact_record(full))


def test_compact_record_is_strict_json_whatever_the_numbers():
    import bench
    full = json.load(open(os.path.join(ROOT, "profiles", "bench_r04c.json")))
    full["value"] = float("nan"); full["roofline"]["achieved"] = float("inf"); full["parity"]["dt_m"] = float("-inf")
    full["online_c5"]["cpu_baseline"]["pose_difference_at_that_point"]["dt_m"] = None
    c = _strict(bench.compact_record(full))
    assert c["value"] is None and c["roofline"]["achieved"] is None and c["parity"]["dt_m"] is None


def test_emit_prints_one_compact_line_on_stdout(capsys, tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    full = json.load(open(os.path.join(ROOT, "profiles", "bench_r04c.json")))
    bench.emit(full)
    cap = capsys.readouterr()
    lines = [l for l in cap.out.splitlines() if l.strip()]
    assert len(lines) == 1
    _check(lines[0])
    assert json.loads(cap.err.strip().splitlines()[-1])["online_c5"]["metric"]            # the full record is on stderr ...
    assert json.load(open(tmp_path / "gpurun_out" / "bench_full.json"))["c4_1gpu"]        # ... and in gpurun_out/


def test_every_traffic_key_the_bench_reads_is_in_traffic_json():
    """`roofline.traffic` comes from profiles/traffic.json (PMC passes of profiles/collect.sh): a kernel renamed since the last collection
    (a template argument more) silently drops its key there and the bench reports `traffic: null`."""
    import re
    src = open(os.path.join(ROOT, "bench.py")).read()
    keys = set(re.findall(r'traffic_of\((.*?), ', src))                      # the key argument: one name, or `"a" if cond else "b"`
    keys = set(k for arg in keys for k in re.findall(r'"([a-z0-9_]+_bytes_per_launch)"', arg))
    assert len(keys) >= 8, keys
    have = json.load(open(os.path.join(ROOT, "profiles", "traffic.json")))
    missing = sorted(k for k in keys if not (isinstance(have.get(k), (int, float)) and have[k] > 0))
    assert not missing, missing


def test_dump_outputs_types_size_cap_and_fixed_sample(tmp_path):
    """`--dump-outputs DIR`: one DIR/<name>.npy per array, float64 kept and every other type as float32; above the cap the same seeded
    row sample of every large array, so that two runs (two builds) compare element for element."""
    import numpy as np
    import bench
    poses = np.random.default_rng(3).random((5000, 12)); used = (poses[:, 0] > 0.5).astype(np.uint8); chi2 = np.array([2.5, 1.25])
    names = bench.dump_outputs(str(tmp_path / "small"), dict(poses=poses, edge_used=used, chi2=chi2))
    assert names == ["chi2", "edge_used", "poses"]
    got = {n: np.load(tmp_path / "small" / (n + ".npy")) for n in names}
    assert got["poses"].dtype == np.float64 and np.array_equal(got["poses"], poses)
    assert got["edge_used"].dtype == np.float32 and np.array_equal(got["edge_used"], used)
    assert np.array_equal(got["chi2"], chi2)
    limit = 200_000
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), dict(poses=poses, edge_used=used, chi2=chi2), limit=limit)
        assert sum(f.stat().st_size for f in (tmp_path / run).iterdir()) <= limit
    for f in ("poses.npy", "poses_rows.npy", "edge_used.npy", "chi2.npy"):
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))
    rows = np.load(tmp_path / "a" / "poses_rows.npy").astype(np.int64)
    assert 0 < len(rows) < len(poses) and np.array_equal(np.load(tmp_path / "a" / "poses.npy"), poses[rows])
    assert np.array_equal(np.load(tmp_path / "a" / "chi2.npy"), chi2)                       # small arrays stay whole


def test_steps_and_dump_outputs_arguments():
    import subprocess
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--steps" in r.stderr
    import bench
    sys.argv, argv = ["bench.py", "--steps", "7", "--warmup", "0", "--dump-outputs", "d"], sys.argv
    try:
        a = bench.parse()
    finally:
        sys.argv = argv
    assert a.steps == 7 and a.warmup == 0 and a.dump_outputs == "d"


def test_dumped_pgo_outputs_are_finite():
    """uzl_pgo_store reports NaN as the error of an edge that did not enter the solve; the dump keeps the errors of the edges that did
    (edge_used, full length, says which), so every dumped value is finite and each error still maps to its input edge."""
    import numpy as np
    import bench
    poses = np.arange(36.).reshape(3, 12)
    err = np.array([np.nan, 0.5, 0.25, np.nan, 1.0]); used = np.array([0, 1, 1, 0, 1], np.uint8)
    o = bench.pgo_outputs((poses, err, used), dict(chi2_initial=4.0, chi2_final=1.5))
    assert sorted(o) == ["chi2", "edge_error", "edge_used", "poses"]
    assert np.array_equal(o["edge_error"], [0.5, 0.25, 1.0]) and np.array_equal(o["edge_used"], used)
    assert np.array_equal(o["chi2"], [4.0, 1.5]) and np.array_equal(o["poses"], poses)
    assert all(np.isfinite(np.asarray(v, np.float64)).all() for v in o.values())


class _FakePgo:
    """Stands in for capi.Pgo in the CPU tests of bench.main(): counts the solves, returns fixed stats."""
    made = []

    def __init__(self, device=0, **cfg):
        import types
        self.cfg = types.SimpleNamespace(pcg_tol=1e-5, preconditioner=1, **cfg)
        self.solves = 0
        _FakePgo.made.append(self)

    def add_graph(self, poses, fixed, edges):
        self.n = len(poses); self.m = len(edges["from"])

    def reset(self):
        pass

    def set_config(self, **cfg):
        pass

    def optimize(self, iterations):
        import time
        time.sleep(0.002)
        self.solves += 1
        return dict(n_edges=self.m, iterations_done=iterations, lm_trials=iterations, pcg_iterations=300, precond_builds=1, chi2_initial=2.0,
                    chi2_final=1.0, structure_ms=0.5, lm_passes=1)

    def store(self):
        import numpy as np
        return np.zeros((self.n, 12)), np.full(self.m, 0.5), np.ones(self.m, np.uint8)

    def close(self):
        pass


def _run_main(monkeypatch, tmp_path, argv):
    import types
    import bench
    import uzliti_slam_amd
    from uzliti_slam_amd import synth
    fake = types.SimpleNamespace(lib=lambda: None, Pgo=_FakePgo)
    monkeypatch.setattr(uzliti_slam_amd, "capi", fake, raising=False)
    monkeypatch.setitem(sys.modules, "uzliti_slam_amd.capi", fake)
    monkeypatch.setattr(synth, "make_pose_graph", lambda n, m, seed=0: dict(nodes_pose=[0] * n, nodes_fixed=[0] * n, edges={"from": [0] * m}))
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    _FakePgo.made = []
    bench.main()


FULL_ONLY = ("roofline", "rooflines", "cpu_baseline", "parity", "first_solve_ms", "repeat_identical", "continued_from_solution", "lm_overhead_ms",
             "streams", "xy_only", "secondary", "batched", "formats", "c4_1gpu", "online_c5", "sharded_c4")


def test_plain_run_solves_only_the_headline_steps(capsys, tmp_path, monkeypatch):
    """Without --full the bench makes one handle and solves 1 (first) + W + N times: no other block, baseline or profiled solve."""
    import numpy as np
    import bench
    monkeypatch.setattr(bench, "full_record", lambda *x: (_ for _ in ()).throw(AssertionError("--full block ran in a plain run")))
    _run_main(monkeypatch, tmp_path, ["--steps", "5", "--warmup", "2", "--dump-outputs", str(tmp_path / "d")])
    assert len(_FakePgo.made) == 1 and _FakePgo.made[0].solves == 1 + 2 + 5
    lines = [l for l in capsys.readouterr().out.splitlines() if l.strip()]
    assert len(lines) == 1
    c = _strict(lines[0])
    assert c["metric"] == "SE(3) edges optimized/sec (node-pairs matched/sec in `secondary`)" and c["unit"] == "edges/s"
    assert c["higher_is_better"] is True and c["dtype"] == "f64" and c["steps"] == 5 and c["warmup"] == 2
    assert c["value"] > 0 and c["ms_per_step"] > 0 and abs(c["value"] * c["ms_per_step"] * 1e-3 - 5000 * 20) < 1e-3 * 5000 * 20
    assert c["config"]["workload"].startswith("BASELINE config 2")
    assert not [k for k in FULL_ONLY if c.get(k)]                            # null: not measured in this run
    assert sorted(f.name for f in (tmp_path / "d").iterdir()) == ["chi2.npy", "edge_error.npy", "edge_used.npy", "poses.npy"]
    assert np.load(tmp_path / "d" / "poses.npy").shape == (1000, 12)


def test_full_run_adds_the_other_blocks_after_the_headline(capsys, tmp_path, monkeypatch):
    import bench
    seen = {}

    def full(capi, synth, ud, dist, dev, a, B, value):
        seen["value"] = value
        return dict(roofline=dict(kernel="k"), cpu_baseline=dict(value=1.0)), []
    monkeypatch.setattr(bench, "full_record", full)
    _run_main(monkeypatch, tmp_path, ["--steps", "3", "--warmup", "1", "--full"])
    c = _strict(capsys.readouterr().out.splitlines()[-1])
    assert c["value"] == round(seen["value"], 1) and c["steps"] == 3
    assert c["roofline"]["kernel"] == "k" and c["cpu_baseline"]["value"] == 1.0
