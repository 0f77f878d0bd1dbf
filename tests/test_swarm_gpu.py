"""The N>1 path on ONE GPU (-m gpu): two processes share GPU 0 and talk over gloo, so the cross-agent exchange, the NetVLAD gate and
the gated cross-agent matching are checked against the oracle without an 8-GPU node (tests/helpers/swarm_worker.py), the block /
gate / half-image kernels are checked against numpy, and bench.py's own --gpus 2 path is run end to end."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _torchrun(script_args, env_extra, timeout=900, merged=False):
    env = dict(os.environ); env.update(env_extra)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port())] + script_args
    if merged:
        r = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=timeout)
        r.stderr = ""
        return r
    return subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)


def _last_line(r):
    """the bench contract: the JSON line is the LAST line of stdout -- callers below run bench.py with stderr merged into stdout (the worst case: RCCL's exit-time banner
    and every warning share the stream with the line), so a line that is not last fails json.loads here"""
    return json.loads(r.stdout.strip().splitlines()[-1])


def _full(j):
    """the full record of a run: the extras file its line names (legs, timelines, per-stage tables, prose)"""
    f = j["extras"]["file"]
    return json.load(open(f if os.path.isabs(f) else os.path.join(ROOT, f)))


def _rank_errors(r):
    """the ranks' own tracebacks (torchrun's summary that follows them is noise)"""
    lines = [l for l in (r.stdout + "\n" + r.stderr).splitlines() if l.startswith("[rank") or "Error" in l or "assert" in l]
    return "\n".join(lines[:60])


def test_world2_cross_agent_matches_equal_oracle():
    r = _torchrun([os.path.join(ROOT, "tests", "helpers", "swarm_worker.py")], {})
    assert r.returncode == 0, _rank_errors(r)
    assert r.stdout.count(" OK: ") == 2, r.stdout[-2000:]


@pytest.mark.parametrize("mode", ["fp32", "int8", "int8-renorm256", "fp32-4lanes", "fp32-4lanes-torch"])
def test_world2_exchange_behind_the_pipe_equals_oracle(mode):
    """The path `bench.py --gpus N` times (round 5): every rank's frames-in-flight pipe with swarm.PipeExchange on a stream of its own one submit behind it
    (d2fe_pipe_device_view -> pack -> all-gather -> gate -> remote matchKNN -> d2fe_pipe_device_release -> D2H): cross-agent match lists and gate decisions against
    the oracle per submit, the pipe's own results bit-identical with and without the exchange beside it."""
    impl = "torch" if mode.endswith("-torch") else "capi"          # capi: d2fe_exchange_* on the lanes' streams (round 6); torch: round 5's Python-driven form, kept as the fallback
    mode = mode.replace("-torch", "")
    lanes = "4" if mode.endswith("-4lanes") else "2"
    r = _torchrun([os.path.join(ROOT, "tests", "helpers", "pipe_exchange_worker.py")], {"PIPE_XCHG_MODE": mode.replace("-4lanes", ""), "PIPE_XCHG_LANES": lanes, "PIPE_XCHG_IMPL": impl})
    assert r.returncode == 0, _rank_errors(r)
    assert r.stdout.count(" OK: ") == 2, r.stdout[-2000:]


@pytest.mark.parametrize("mode,overlap", [("gated", "0"), ("all2all", "0"), ("all2all", "1")])
def test_world2_quadcam_swarm_equals_oracle(mode, overlap):
    """BASELINE configs[4] on one GPU: two quadcam agents, one block per view, the FOURCORNER_FISHEYE gate, view x view matching; overlap = 1: the exchange on
    a stream of its own behind a snapshot, with the next chain step overwriting the chain's buffers beside it (QuadSwarm.step_overlapped, what bench.py times)."""
    r = _torchrun([os.path.join(ROOT, "tests", "helpers", "quad_swarm_worker.py")], {"QUAD_SWARM_MODE": mode, "QUAD_SWARM_OVERLAP": overlap})
    assert r.returncode == 0, _rank_errors(r)
    assert r.stdout.count(" OK: ") == 2, r.stdout[-2000:]


def test_bench_self_launches_n_ranks_from_a_bare_shell():
    """`python bench.py --gpus 2` with no WORLD_SIZE in the environment (how the driver calls it) re-launches itself as 2 ranks; the record
    carries the process group's own evidence.  gloo: RCCL does not put two ranks on one device."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["D2FE_BENCH_BACKEND"] = "gloo"
    for extra, key in ((["--frames", "2"], "netvlad_gate"), (["--workload", "quadcam", "--frames", "4"], "cross_agent")):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--single-mode",
                            "--no-cpu-baseline"] + extra, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
        assert r.returncode == 0, r.stdout[-3000:]
        j = _last_line(r)
        assert "roofline" in j and "cpu_baseline" in j and len(r.stdout.strip().splitlines()[-1]) < 6000
        j = _full(j)
        assert j["n_gpus"] == 2 and j["value"] > 0 and key in j
        e = j["rccl"]
        assert e["backend"] == "gloo" and e["world_size"] == 2 and e["allreduce_sum_of_ranks"] == 1.0 and len(e["ranks"]) == 2
        assert {x["rank"] for x in e["ranks"]} == {0, 1} and len({x["pid"] for x in e["ranks"]}) == 2
    assert j["cross_agent"]["view_pairs_per_step_per_gpu"] == 16 and j["netvlad_gate"]["jobs"] == 1


def test_bench_gpus2_path_runs_under_gloo():
    r = _torchrun([os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--frames", "2", "--single-mode", "--no-cpu-baseline"],
                  {"D2FE_BENCH_BACKEND": "gloo"}, merged=True)
    assert r.returncode == 0, r.stdout[-3000:]
    j = _full(_last_line(r))
    assert j["n_gpus"] == 2 and j["value"] > 0 and j["config"]["match_pairs_per_step_per_gpu"] == 2 * 2 + 2
    assert j["netvlad_gate"]["pairs"] == 2 and 0 <= j["netvlad_gate"]["passing_netvlad_gate"] <= 2
    assert j["avg_matches_per_pair"] > 1


def test_pack_blocks_and_gate_kernels():
    import torch
    from d2slam_amd import api
    dev = torch.device("cuda", 0)
    fe = api.FrontEnd(api.SuperPointConfig(max_keypoints=50, input_width=64, input_height=64, max_batch=1))
    cap, G, rows = 50, 64, 6
    rng = np.random.RandomState(0)
    desc = rng.randn(rows, cap, 256).astype(np.float32); kps = rng.rand(rows, cap, 2).astype(np.float32) * 100
    sc = rng.rand(rows, cap).astype(np.float32); n = np.array([50, 0, 7, 33, 60, 1], np.int32)       # 60 > cap: clamped
    g = rng.randn(3, G).astype(np.float32)
    BLK = api.block_words(cap, G)
    t = lambda a: torch.from_numpy(a).to(dev)
    d_desc, d_kps, d_sc, d_n, d_g = t(desc), t(kps), t(sc), t(n), t(g)
    blocks = torch.full((3, BLK), 7.0, device=dev)
    fe.pack_blocks_device(d_desc.data_ptr(), d_kps.data_ptr(), d_sc.data_ptr(), d_n.data_ptr(), d_g.data_ptr(), 1, 2, 3, cap, G, blocks.data_ptr())
    fe.sync(); torch.cuda.synchronize()
    b = blocks.cpu().numpy()
    off = {f: api.block_field_offset(cap, G, f) for f in ("desc", "kps", "scores", "netvlad", "n")}
    for f in range(3):
        row = 1 + 2 * f; k = min(int(n[row]), cap)
        exp = np.zeros(BLK, np.float32)
        exp[:k * 256] = desc[row, :k].reshape(-1); exp[off["kps"]:off["kps"] + 2 * k] = kps[row, :k].reshape(-1)
        exp[off["scores"]:off["scores"] + k] = sc[row, :k]; exp[off["netvlad"]:off["netvlad"] + G] = g[f]
        exp.view(np.int32)[off["n"]] = k
        assert np.array_equal(b[f].view(np.int32), exp.view(np.int32)), f
    # gate: pairs (q row, db row) with strided rows
    q = rng.randn(4, G).astype(np.float32); q /= np.linalg.norm(q, axis=1, keepdims=True)
    db = np.zeros((5, 2 * G), np.float32); db[:, :G] = q[[0, 1, 2, 3, 0]] + 0.3 * rng.randn(5, G).astype(np.float32)
    db[:, :G] /= np.linalg.norm(db[:, :G], axis=1, keepdims=True)
    pq = np.array([0, 1, 2, 3, 1, 2], np.int32); pd = np.array([0, 1, 2, 3, 4, 0], np.int32)
    sims = np.array([np.dot(q[a], db[c, :G]) for a, c in zip(pq, pd)])
    thres = 0.5
    cnt = torch.full((6,), 9, dtype=torch.int32, device=dev); pas = torch.zeros(6, dtype=torch.int32, device=dev)
    gs = torch.zeros(6, device=dev); gn = torch.zeros(1, dtype=torch.int32, device=dev)
    d_q, d_db, d_pq, d_pd = t(q), t(db), t(pq), t(pd)        # keep the device tensors alive across the launch
    fe.gate_pairs_device(d_q.data_ptr(), G, d_db.data_ptr(), 2 * G, G, d_pq.data_ptr(), d_pd.data_ptr(), 6, thres, d_cnt_inout=cnt.data_ptr(),
                         d_pass=pas.data_ptr(), d_sims=gs.data_ptr(), d_n_pass=gn.data_ptr())
    fe.sync(); torch.cuda.synchronize()
    assert np.abs(gs.cpu().numpy() - sims).max() <= 1e-5
    exp_pass = (sims >= thres).astype(np.int32)
    assert np.array_equal(pas.cpu().numpy(), exp_pass) and int(gn.item()) == exp_pass.sum()
    assert np.array_equal(cnt.cpu().numpy(), np.where(exp_pass == 1, 9, 0))
    fe.close()


def test_rccl_single_rank_collectives():
    """The nccl (= RCCL) calls of bench.py's --gpus N path -- init with device_id, the exchange all-gather on a side stream, barrier,
    all-reduce MAX -- on the one GPU this box has (the world-2 tests above run the same path over gloo)."""
    env = dict(os.environ); env["MASTER_PORT"] = str(_free_port())
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_rccl_1rank.py")], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "RCCL 1-rank OK" in r.stdout, (r.stdout + r.stderr)[-2000:]


def _bare_env(**extra):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(extra)
    return env


def test_bench_default_line_contract_and_one_gpu_rccl_loopback_leg(tmp_path):
    """`python bench.py --full` (fewer steps / CPU iterations, the long legs off), stderr MERGED into stdout: the JSON line is the last line although the run
    creates and destroys a one-rank RCCL communicator (whose banner C stdio flushes at exit -- round 5's line was lost to it), it is < 6 KB and carries `roofline` and
    `cpu_baseline` by the SURVEY 8(d) protocol; the other legs are in the extras file it names.  `exchange_on_one_gpu_rccl` there: the N > 1 exchange sequence behind the
    value step over the one-rank communicator (loopback), with vs without; it must run (no "error") and cost a few per cent at most."""
    ex = str(tmp_path / "extras.json")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--steps", "6", "--warmup", "2", "--frames", "8", "--cpu-iterations", "3", "--no-latency", "--no-batch-curve",
                        "--no-live-traffic", "--no-width-sensitivity", "--no-parity-study"], cwd=ROOT, env=_bare_env(D2FE_BENCH_EXTRAS=ex),
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout[-3000:]
    last = r.stdout.strip().splitlines()[-1]
    j = json.loads(last)
    assert len(last) < 6000 and j["n_gpus"] == 1 and j["value"] > 0
    assert j["roofline"]["bound"] == "mfma" and 0 < j["roofline"]["frac"] < 1 and j["roofline"]["avg_launch_ms"] > 0
    cb = j["cpu_baseline"]
    assert cb["kind"] == "port" and cb["value"] > 0 and cb["all_cores"]["timed_iterations"] == 3 and cb["all_cores"]["warmup_iterations"] == 5 and cb["single_thread"]["threads"] == 1
    assert j["parity"]["keypoints_equal"] and j["parity"]["scores_equal"]
    assert j["extras"]["file"] == ex and "exchange_on_one_gpu_rccl" in j["extras"]["keys"]
    full = json.load(open(ex))
    assert full["value"] == j["value"] and "ms_per_stereo_frame" in full["cpu_baseline"]["all_cores"]
    e = full["exchange_on_one_gpu_rccl"]
    assert "error" not in e, e
    assert e["backend"] == "nccl" and e["value_with_exchange"] > 0 and e["step_timeline_ms"]["all_gather"] > 0
    assert e["exchange_cost_frac_of_step"] < 0.25, e      # ~2 % at 32 frames per submit; small steps on a shared box are noisier


def test_bench_plain_run_times_value_only_and_dumps_identical_outputs(tmp_path):
    """`python bench.py --gpus 1 --steps N --warmup W` without --full: the headline step only (no CPU baseline, no secondary leg), and --dump-outputs writes what the
    last timed step delivered -- the same arrays, bit for bit, from two runs with the same arguments."""
    runs = []
    for i in range(2):
        d = str(tmp_path / ("out%d" % i))
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "2", "--frames", "4", "--dump-outputs", d], cwd=ROOT,
                           env=_bare_env(D2FE_BENCH_EXTRAS=str(tmp_path / ("extras%d.json" % i))), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-3000:]
        j = _last_line(r)
        assert j["steps"] == 4 and j["ms_per_step"] > 0 and j["higher_is_better"] is True and j["dtype"] == "f32" and j["unit"] == "stereo_frames/s"
        assert abs(j["value"] - 4 * 1e3 / j["ms_per_step"]) / j["value"] < 0.01
        assert j["cpu_baseline"] is None and "parity" not in j
        full = _full(j)
        for k in ("configs1", "exact_mode", "fast_mode", "batch_curve", "latency", "quadcam", "device_resident", "index_parity_in_run", "exchange_on_one_gpu_rccl"):
            assert k not in full, k
        runs.append({n[:-4]: np.load(os.path.join(d, n)) for n in os.listdir(d)})
    a, b = runs
    assert sorted(a) == sorted(["kps_xy", "scores", "desc", "n_kp", "netvlad", "lr_q", "lr_t", "lr_dist", "lr_n", "prev_q", "prev_t", "prev_dist", "prev_n"])
    assert a["desc"].shape == (8, 200, 256) and a["netvlad"].shape[0] == 4 and a["lr_n"].shape == (4,)
    for k in a:
        assert a[k].dtype in (np.float32, np.float64) and np.array_equal(a[k], b[k]), k
    n = a["n_kp"].astype(np.int64)
    assert (n > 0).all() and all(not a["desc"][i, n[i]:].any() for i in range(8))
    assert np.allclose(np.linalg.norm(a["desc"][0, :n[0]], axis=1), 1.0, atol=1e-4)


def test_bench_force_dist_sends_one_rank_through_the_n_gpu_path(tmp_path):
    """--force-dist: --gpus 1 through self_launch -> torch.distributed.run -> init_process_group("nccl", device_id) -> collective_evidence -> PipeExchange
    (loopback) -> destroy_process_group with the N > 1 lane count; the line is still the last line of the merged stream and says what it ran."""
    ex = str(tmp_path / "extras.json")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--force-dist", "--full", "--steps", "6", "--warmup", "2", "--frames", "8", "--single-mode"], cwd=ROOT,
                       env=_bare_env(D2FE_BENCH_EXTRAS=ex), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:]
    j = _last_line(r)
    assert j["n_gpus"] == 1 and j["value"] > 0 and "roofline" in j and "cpu_baseline" in j
    e = j["rccl"]
    assert e["is_rccl"] and e["backend"] == "nccl" and e["world_size"] == 1 and e["allreduce_sum_of_ranks"] == 0.0
    full = json.load(open(ex))
    x = full["exchange"]
    assert x["cross_agent_pairs_per_step_per_gpu"] == 8 and x["step_timeline_ms"]["all_gather"] > 0 and x["value_without_exchange"] > 0
    assert full["netvlad_gate"]["pairs"] == 8 and full["netvlad_gate"]["passing_netvlad_gate"] == 8      # every frame against itself
    assert "--force-dist" in full["config"]["workload"]


def test_int8_exchange_blocks_vs_reference_codec():
    """The int8 wire format of the exchange block: bytes equal the reference's own toLCM quantisation (oracle/_ref, compiled in place) on the
    frame's n x 256 descriptor vector and on the NetVLAD vector; the decoded fp32 block equals the reference's LCM-constructor decode
    (q/127.0, the first n 32-float segments re-normalised, whole-vector NetVLAD normalisation)."""
    import torch
    from d2slam_amd import api, swarm
    from oracle import oracle as orc, ref as spref
    orc.build()
    dev = torch.device("cuda", 0)
    fe = api.FrontEnd(api.SuperPointConfig(max_keypoints=50, input_width=64, input_height=64, max_batch=1))
    cap, G, rows = 48, 128, 5
    rng = np.random.RandomState(2)
    desc = rng.randn(rows, cap, 256).astype(np.float32); desc /= np.linalg.norm(desc, axis=2, keepdims=True)
    kps = (rng.rand(rows, cap, 2) * 100).astype(np.float32); n = np.array([48, 0, 7, 33, 90], np.int32)      # 90 > cap: clamped
    g = rng.randn(rows, G).astype(np.float32); g /= np.linalg.norm(g, axis=1, keepdims=True)
    BB = api.block_bytes_int8(cap, G); BLK = api.block_words(cap, G)
    assert BB == swarm.block_bytes_int8(cap, G) and BB * 3.5 < 4 * BLK
    t = lambda a: torch.from_numpy(a).to(dev)
    d_desc, d_kps, d_n, d_g = t(desc), t(kps), t(n), t(g)
    bq = torch.full((rows, BB), 7, dtype=torch.int8, device=dev)
    torch.cuda.synchronize()      # the library launches on the handle's own non-blocking stream, which does not wait for torch's fills on the default stream
    fe.pack_blocks_int8_device(d_desc.data_ptr(), d_kps.data_ptr(), d_n.data_ptr(), d_g.data_ptr(), 0, 1, rows, cap, G, bq.data_ptr())
    for renorm in (0, 1):
        out = torch.full((rows, BLK), 7.0, device=dev)
        torch.cuda.synchronize()
        fe.unpack_blocks_int8_device(bq.data_ptr(), rows, cap, G, out.data_ptr(), renorm=renorm)
        fe.sync(); torch.cuda.synchronize()
        q = bq.cpu().numpy(); o = out.cpu().numpy()
        off = {f: api.block_field_offset(cap, G, f) for f in ("desc", "kps", "scores", "netvlad", "n")}
        for f in range(rows):
            k = min(int(n[f]), cap)
            have_ref = spref.available()
            ql = (spref.quant_landmarks if have_ref else orc.quant_int8)(desc[f, :k].reshape(-1)) if k else np.zeros(0, np.int8)
            qn = spref.quant_netvlad(g[f]) if have_ref else orc.quant_int8(g[f], double_max=True)
            assert np.array_equal(q[f, :k * 256], ql) and not q[f, k * 256:cap * 256].any()
            assert np.array_equal(q[f, cap * 256:cap * 256 + G], qn)
            assert np.array_equal(q[f, cap * 256 + G:cap * 256 + G + cap * 8].view(np.float32)[:2 * k], kps[f, :k].reshape(-1))
            assert int(q[f, cap * 256 + G + cap * 8:cap * 256 + G + cap * 8 + 4].view(np.int32)[0]) == k
            if renorm == 0:
                rl, rn = (spref.dequant(ql, k, qn) if have_ref else (orc.dequant_int8(ql, k) if k else np.zeros(0, np.float32), orc.dequant_int8(qn, -1)))
            else:
                x = (ql.astype(np.float64) / 127.0).astype(np.float32).reshape(k, 256)
                rl = (x / np.linalg.norm(x, axis=1, keepdims=True)).reshape(-1) if k else np.zeros(0, np.float32)
                rn = orc.dequant_int8(qn, -1)
            assert np.abs(o[f, :k * 256] - rl).max(initial=0) <= 1e-6 and not o[f, k * 256:off["kps"]].any()
            assert np.abs(o[f, off["netvlad"]:off["netvlad"] + G] - rn).max() <= 1e-6
            assert np.array_equal(o[f, off["kps"]:off["kps"] + 2 * k], kps[f, :k].reshape(-1)) and not o[f, off["scores"]:off["netvlad"]].any()
            assert int(o[f].view(np.int32)[off["n"]]) == k
            if renorm == 0 and k >= 16:
                # the reference's decode: rows < k/8 are unit per 32-float segment (norm sqrt(8)), the rest stay scaled by 1/max|x|
                nr = np.linalg.norm(o[f, :k * 256].reshape(k, 256), axis=1)
                assert np.abs(nr[:k // 8] - np.sqrt(8.0)).max() < 1e-4 and nr[k // 8 + 1:].min() > 1.5
    fe.close()


def test_bench_gpus2_one_frame_per_step_timeline():
    """The real swarm cadence (VERDICT r03 #6b): ONE stereo frame per agent and step.  Two ranks share the GPU under gloo (the all-gather is staged
    through the host there, so ITS time says nothing about xGMI); what is held to a budget is everything this library adds on the device beside
    it: packing the blocks and decode / count fix-up / NetVLAD gate, from HIP events on the exchange's stream."""
    r = _torchrun([os.path.join(ROOT, "bench.py"), "--gpus", "2", "--full", "--steps", "6", "--warmup", "2", "--frames", "1", "--single-mode", "--no-cpu-baseline"],
                  {"D2FE_BENCH_BACKEND": "gloo"}, merged=True)
    assert r.returncode == 0, r.stdout[-3000:]
    j = _full(_last_line(r))
    assert j["n_gpus"] == 2 and j["config"]["frames_per_step_per_gpu"] == 1 and j["config"]["match_pairs_per_step_per_gpu"] == 3
    tl = j["exchange"]["step_timeline_ms"]
    # budget: 0.35 ms of a ~1 ms step, without the collective (round 5: the exchange stream runs BESIDE the lanes' launches of the next submit and beside
    # the other rank's work on the same GPU, so an entry is a wall time on a shared device: twice the solo budget)
    assert 0 < tl["pack_blocks"] <= 0.20 and 0 < tl["decode_counts_gate"] <= 0.50, tl
    assert tl["all_gather"] > 0 and tl["match_remote"] > 0
    assert j["netvlad_gate"]["pairs"] == 1
    # the N > 1 step is the N = 1 step (the pipe) plus the exchange stream: same API string, and the cost of the exchange is reported against the same ranks without it
    assert j["config"]["same_path_for_every_n_gpus"] is True and "d2fe_pipe_submit" in j["config"]["api"]
    assert j["exchange"]["ms_per_step_without_exchange"] > 0 and "overlapped" in j["exchange"]


def test_bench_int8_exchange_runs_under_gloo():
    r = _torchrun([os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--frames", "2", "--single-mode", "--no-cpu-baseline",
                   "--exchange", "int8"], {"D2FE_BENCH_BACKEND": "gloo"}, merged=True)
    assert r.returncode == 0, r.stdout[-3000:]
    j = _full(_last_line(r))
    assert j["exchange"]["wire_precision"] == "int8" and j["exchange"]["block_bytes"] * 3.5 < 4 * 56064
    assert j["exchange"]["avg_cross_agent_matches_per_pair"] >= 0
    # the quadcam swarm over int8 blocks (one per view)
    r = _torchrun([os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--frames", "4", "--workload", "quadcam",
                   "--exchange", "int8"], {"D2FE_BENCH_BACKEND": "gloo"}, merged=True)
    assert r.returncode == 0, r.stdout[-3000:]
    j = _full(_last_line(r))
    assert j["cross_agent"]["wire_precision"] == "int8" and j["cross_agent"]["view_pairs_per_step_per_gpu"] == 16 and j["n_gpus"] == 2
