"""bench.py's host-side helpers (no GPU): the cross-mode disagreement count, the traffic figure read from the committed PMC summary,
the roofline arithmetic of the dominant kernel."""
import os

import numpy as np

import bench


def _sel(F, CAP):
    NI = 2 * F
    kidx = np.arange((NI + F) * CAP).reshape(NI + F, CAP).astype(np.int32)
    return dict(kidx=kidx, cnt=np.full(3 * F, CAP, np.int32), mq=np.tile(np.arange(CAP), (2 * F, 1)), mt=np.tile(np.arange(CAP), (2 * F, 1)),
                mn=np.full(2 * F, CAP), a_row=[0, 0, 1, 1], b_row=[2, 4, 3, 5])


def test_mode_disagreement_counts_symmetric_differences():
    F, CAP = 2, 5
    a = _sel(F, CAP)
    b = {k: (v.copy() if hasattr(v, "copy") else list(v)) for k, v in a.items()}
    d = bench.mode_disagreement(a, b, F)
    assert d["keypoints_in_one_mode_only"] == 0 and d["matches_in_one_mode_only"] == 0 and d["keypoints_exact_mode"] == 20
    b["kidx"][0, 0] = 999            # image 0: one keypoint differs -> 2 in the symmetric difference; its matches change in both pairs of frame 0
    b["mt"][1, 0] = 3                # pair 1 (L0 <-> prev L0): one more match differs
    d = bench.mode_disagreement(a, b, F)
    assert d["keypoints_in_one_mode_only"] == 2 and d["images_with_any_keypoint_difference"] == 1
    assert d["matches_in_one_mode_only"] == 4 and d["left_right_matches_in_one_mode_only"] == 2
    # order inside a keypoint list does not matter: matches are compared as raster-index pairs
    c = {k: (v.copy() if hasattr(v, "copy") else list(v)) for k, v in a.items()}
    perm = np.array([4, 3, 2, 1, 0])
    c["kidx"][0] = a["kidx"][0][perm]; c["mq"][0] = perm.argsort()[a["mq"][0]]; c["mq"][1] = perm.argsort()[a["mq"][1]]
    d = bench.mode_disagreement(a, c, F)
    assert d["keypoints_in_one_mode_only"] == 0 and d["matches_in_one_mode_only"] == 0


def test_roofline_arithmetic_and_profiled_traffic():
    r = bench.conv1b_roofline("wino", 5.65, 20, 64, True)
    items = 64 * 60 * 40
    assert r["executed_mfma_flop_per_launch"] == items * 1084 * 4096.0 and abs(r["frac"] - r["achieved"] / 157.3) < 1e-3
    assert abs(r["algorithmic_flop_per_launch"] - 64 * 2.0 * 480 * 640 * 64 * 576) < 1 and r["frac_algorithmic"] > 1.0
    assert r["compulsory_bytes_per_launch"] == 64 * (480 * 640 + 240 * 320 * 64 * 4)
    path = os.path.join(bench.ROOT, "profiles", "r03_wino_rocprofv3_summary.txt")
    if os.path.exists(path):
        assert 1.0 < r["traffic"] / r["compulsory_bytes_per_launch"] < 1.3 and "FETCH_SIZE" in r["traffic_note"]
    e = bench.conv1b_roofline("f32", 10.6, 20, 64, True)
    assert abs(e["frac"] - e["algorithmic_flop_per_launch"] / 10.6e-3 / 1e12 / 157.3) < 1e-3


def test_live_traffic_parses_a_counter_pass_and_never_recurses(tmp_path, monkeypatch):
    """bench.live_traffic(): the child passes never start passes of their own; a pass is averaged per dispatch of the named kernel and combined as
    (2 x FETCH_SIZE + WRITE_SIZE) KiB; no rocprofv3 or a failed pass -> None (the committed profile is quoted instead)."""
    import subprocess
    monkeypatch.setenv("D2FE_BENCH_CHILD", "1")
    assert bench.live_traffic("conv_wino_kernel") is None
    monkeypatch.delenv("D2FE_BENCH_CHILD")
    calls = []

    def fake_run(cmd, cwd=None, env=None, capture_output=None, text=None, timeout=None):
        ctr = cmd[cmd.index("--pmc") + 1]; d = cmd[cmd.index("-d") + 1]
        assert env["D2FE_BENCH_CHILD"] == "1" and "--single-mode" in cmd and cmd[cmd.index("--lanes") + 1] == "1"
        calls.append(ctr)
        os.makedirs(os.path.join(d, "host", "1"), exist_ok=True)
        with open(os.path.join(d, "host", "1", "p_counter_collection.csv"), "w") as f:
            f.write("Kernel_Name,Counter_Name,Counter_Value\n")
            for v in (100.0, 300.0):
                f.write('"void d2fe::conv_wino_kernel<64, true, true, 0, 1, true, 2>(ConvArgs, int, int, int, int)",%s,%f\n' % (ctr, v if ctr == "FETCH_SIZE" else 10 * v))
            f.write('"other_kernel",%s,5.0\n' % ctr)
        return subprocess.CompletedProcess(cmd, 0, "", "")

    monkeypatch.setattr(bench.shutil if hasattr(bench, "shutil") else __import__("shutil"), "which", lambda n: "/bin/true")
    monkeypatch.setattr(subprocess, "run", fake_run)
    r = bench.live_traffic("conv_wino_kernel<64, true, true, 0, 1, true")
    assert calls == ["FETCH_SIZE", "WRITE_SIZE"]
    assert r["traffic"] == int((2 * 200.0 + 2000.0) * 1024) and r["counters"]["dispatches_averaged"] == [2, 2]
    monkeypatch.setattr(subprocess, "run", lambda *a, **k: subprocess.CompletedProcess(a, 1, "", "boom"))
    assert bench.live_traffic("conv_wino_kernel") is None


def test_step_roofline_and_flags():
    """`step_roofline`: executed matrix-pipe FLOPs of the whole step / wall time / peak.  The analytic per-image count of the Winograd mode must agree with what the
    committed profile measured (SQ_INSTS_MFMA summed over a 64-image step: 3.46e8 x 4096 = 1.42 TFLOP incl. NetVLAD + matcher), and the r04 step (13.086 ms)
    must come out at the judge's 0.69-0.71."""
    g = bench.sp_executed_gflop_per_image("wino")
    assert 22.0 < g < 22.8
    assert abs(bench.sp_executed_gflop_per_image("f32") - (0.354 + 48.123 + 0.44)) < 0.05          # the direct layers + convPb + the sparse head
    assert abs(bench.sp_executed_gflop_per_image("f16x2") - 3 * bench.sp_executed_gflop_per_image("f32")) < 1e-9
    r = bench.step_roofline("wino", 32, 13.086, True, 64)
    # 1.435 SuperPoint (the profile's SQ_INSTS_MFMA sum) + 0.079 NetVLAD at the 0.75 width (0.021 at round 5's 0.35) + 0.003 matcher
    assert abs(r["executed_mfma_tflop_per_step"] - 1.517) < 0.02 and abs(r["superpoint"] - 1.435) < 0.01 and 0.70 < r["frac"] < 0.76 and r["peak"] == 157.3
    assert abs(r["superpoint"] + r["netvlad"] + r["matcher"] - r["executed_mfma_tflop_per_step"]) < 1e-3
    assert r["algorithmic_tflop_per_step"] > r["executed_mfma_tflop_per_step"]
    e = bench.step_roofline("f32", 32, 24.7, True, 64)
    assert 0.78 < e["frac"] < 0.90                                                                  # the exact mode: 0.81 executed (sparse descriptor head), 0.86 on the 52.1 GFLOP algorithmic count
    f = bench.step_roofline("f16x2", 32, 10.2, True, 64)
    assert 0.3 < f["frac"] < 0.5
    w = bench.flag_above_peak(bench.conv1b_roofline("wino", 5.5, 20, 64, True))
    assert w["frac_algorithmic"] > 1 and "16/36" in w["algorithmic_above_peak"] and w["frac"] < 1
    assert "algorithmic_above_peak" not in bench.flag_above_peak(bench.conv1b_roofline("f32", 22.0, 20, 64, True))
    assert bench.build_record()["recorded"] in (True, False)


def test_netvlad_flop_table():
    from d2slam_amd import netvlad as nvm
    assert abs(nvm.arch_flops(0.35) / 1e9 - 0.666) < 0.005 and abs(nvm.arch_flops(0.35, head=True) / 1e9 - 0.769) < 0.005
    assert nvm.arch_flops(0.5) < nvm.arch_flops(0.75) < nvm.arch_flops(1.0)
    assert abs(nvm.arch_flops() / 1e9 - 2.478) < 0.005 and nvm.DEPTH_MULTIPLIER == 0.75          # SURVEY A9's width is the default everywhere
    assert abs(bench.NV_FLOP_PER_IMG / nvm.arch_flops(0.75) - 1.0) < 1e-6


def test_json_line_is_the_last_thing_on_stdout_even_with_buffered_c_stdio_and_merged_stderr(tmp_path):
    """The driver's contract: a library that prints through C stdio (RCCL's version banner: buffered on a pipe, flushed at process exit) must not land
    behind the JSON line -- neither on stdout alone nor when the caller merges stderr into stdout -- and nothing printed after the line may reach either stream."""
    import json
    import subprocess
    import sys
    prog = ("import ctypes, sys, os\n"
            "sys.path.insert(0, %r)\n"
            "import bench\n"
            "libc = ctypes.CDLL(None)\n"
            "bench.claim_stdout()\n"
            "libc.printf(b'RCCL version : banner through C stdio\\n')\n"      # stays in libc's buffer until somebody flushes it
            "print('python print before the line')\n"
            "bench.emit_line({'metric': 'm', 'value': 1.5, 'roofline': {'frac': 0.5}, 'cpu_baseline': None})\n"
            "libc.printf(b'Librccl path : printed at teardown\\n')\n"
            "print('python print after the line'); sys.stderr.write('stderr after the line\\n')\n" % bench.ROOT)
    for merged in (False, True):
        r = subprocess.run([sys.executable, "-c", prog], stdout=subprocess.PIPE, stderr=subprocess.STDOUT if merged else subprocess.PIPE, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + (r.stderr or "")
        lines = r.stdout.strip().splitlines()
        j = json.loads(lines[-1])
        assert j["value"] == 1.5 and j["roofline"]["frac"] == 0.5
        assert "after the line" not in r.stdout and "teardown" not in r.stdout
        if merged:
            assert any("banner through C stdio" in l for l in lines[:-1]) and any("before the line" in l for l in lines[:-1])
        else:
            assert lines == [lines[-1]] and "banner through C stdio" in r.stderr


def test_headline_fits_the_tail_and_names_the_extras_file(tmp_path, monkeypatch):
    """the line keeps the contract's keys + roofline + cpu_baseline in < 6 KB whatever the full record holds; everything else is in the file the line names"""
    import json
    monkeypatch.setenv("D2FE_BENCH_EXTRAS", str(tmp_path / "extras.json"))
    prose = "x" * 900
    full = {"metric": "m", "value": 2.0, "unit": "u", "n_gpus": 8, "steps": 3, "warmup": 1, "ms_per_step": 1.0, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f32", "data": "synthetic", "config": {"workload": "w" * 500, "note": prose, "lanes": 4},
            "roofline": {"bound": "mfma", "achieved": 1.0, "peak": 2.0, "unit": "TFLOP/s", "frac": 0.5, "traffic": 7, "note": prose, "kernel": "k"},
            "cpu_baseline": {"value": 3.0, "unit": "u", "cores": 32, "kind": "port", "sample": "s" * 400,
                             "all_cores": {"threads": 32, "timed_iterations": 50, "ms_per_stereo_frame": {"conv": {"median": 1.0, "p95": 2.0}}},
                             "single_thread": {"threads": 1, "timed_iterations": 50, "ms_per_stereo_frame": {"conv": {"median": 1.0, "p95": 2.0}}}, "fmaf_oracle": {"value": 1}},
            "step_roofline": {"frac": 0.7}, "parity": {"keypoints_equal": True},
            "rccl": {"backend": "nccl", "is_rccl": True, "world_size": 8, "ranks": [{"rank": i, "uuid": "u" * 40, "name": "AMD Instinct MI355X"} for i in range(8)]},
            "exchange": {"step_timeline_ms": {k: 0.1 for k in "abcdefgh"}, "note": prose}, "batch_curve": {"points": [{"note": prose}] * 30}, "latency": {"a": prose}}
    line, path = bench.headline(full)
    assert path == str(tmp_path / "extras.json") and json.load(open(path))["batch_curve"]["points"][0]["note"] == prose
    txt = json.dumps(line)
    assert len(txt) < bench.LINE_BUDGET
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in line, k
    assert line["roofline"]["frac"] == 0.5 and line["roofline"]["traffic"] == 7 and "note" not in line["roofline"]
    assert line["cpu_baseline"]["all_cores"]["timed_iterations"] == 50 and "ms_per_stereo_frame" not in line["cpu_baseline"]["all_cores"]
    assert line["config"]["workload"].startswith("www") and len(line["config"]["workload"]) <= 320
    assert "batch_curve" not in line and "batch_curve" in line["extras"]["keys"] and line["extras"]["file"].endswith("extras.json")
    assert line["rccl"]["world_size"] == 8 and isinstance(line["rccl"]["ranks"], str)
    # a run without a CPU baseline / roofline still carries the keys (null)
    line2, _ = bench.headline({"metric": "m", "value": 1.0})
    assert line2["cpu_baseline"] is None and line2["roofline"] is None and line2["vs_baseline"] is None


def test_dump_outputs_zeroes_rows_past_the_counts_and_fits_the_budget(tmp_path):
    """--dump-outputs: one .npy per delivered array, float32 for floats and float64 for counts / indices (exact), rows past an image's or pair's count zeroed;
    above the budget the large arrays become the same seeded sample on every call."""
    rng = np.random.RandomState(1)
    I, F, C, D, G = 4, 2, 5, 8, 6
    res = {"kps_xy": rng.rand(I, C, 2).astype(np.float32), "scores": rng.rand(I, C).astype(np.float32), "desc": rng.rand(I, C, D).astype(np.float32),
           "n_kp": np.array([5, 0, 3, 9], np.int32), "netvlad": rng.rand(F, G).astype(np.float32), "lr_q": rng.randint(0, C, (F, C)).astype(np.int32),
           "lr_t": rng.randint(0, C, (F, C)).astype(np.int32), "lr_dist": rng.rand(F, C).astype(np.float32), "lr_n": np.array([2, 5], np.int32),
           "prev_q": rng.randint(0, C, (F, C)).astype(np.int32), "prev_t": rng.randint(0, C, (F, C)).astype(np.int32), "prev_dist": rng.rand(F, C).astype(np.float32),
           "prev_n": np.array([0, 1], np.int32), "unused": None}
    rec = bench.dump_outputs(str(tmp_path / "a"), res)
    got = {n[:-4]: np.load(str(tmp_path / "a" / n)) for n in os.listdir(str(tmp_path / "a"))}
    assert sorted(got) == rec["arrays"] == sorted(k for k in res if k != "unused") and rec["sampled"] is None
    assert got["desc"].dtype == np.float32 and got["n_kp"].dtype == np.float64 and got["lr_q"].dtype == np.float64
    assert np.array_equal(got["n_kp"], [5, 0, 3, 9]) and np.array_equal(got["netvlad"], res["netvlad"])
    assert np.array_equal(got["desc"][0], res["desc"][0]) and np.array_equal(got["desc"][3], res["desc"][3]) and not got["desc"][1].any()
    assert np.array_equal(got["desc"][2, :3], res["desc"][2, :3]) and not got["desc"][2, 3:].any() and not got["kps_xy"][2, 3:].any() and not got["scores"][1].any()
    assert np.array_equal(got["lr_q"][0, :2], res["lr_q"][0, :2]) and not got["lr_q"][0, 2:].any() and np.array_equal(got["lr_t"][1], res["lr_t"][1])
    assert not got["prev_dist"][0].any() and np.array_equal(got["prev_dist"][1, :1], res["prev_dist"][1, :1])
    big = dict(res, desc=rng.rand(I, C, 20000).astype(np.float32))          # 1.6 MB: over a 1 MiB + small budget
    budget = (1 << 20) + 4096
    r1 = bench.dump_outputs(str(tmp_path / "b"), big, budget=budget)
    r2 = bench.dump_outputs(str(tmp_path / "c"), big, budget=budget)
    assert r1["bytes"] <= budget and list(r1["sampled"]) == ["desc"]
    s1, s2 = np.load(str(tmp_path / "b" / "desc.npy")), np.load(str(tmp_path / "c" / "desc.npy"))
    assert s1.ndim == 1 and np.array_equal(s1, s2) and s1.nbytes < big["desc"].nbytes
