"""The float64 NetVLAD reference and the case table of tests/test_netvlad_shapes.py, checked without a GPU: the reference against the oracle, the table against
the execution plan and the compiled shape lists (d2fe_debug_netvlad_plan / d2fe_debug_netvlad_shapes of the development library), the clamp shares of the
synthetic weights, and the comparator against deliberately wrong kernels."""
import numpy as np
import pytest

from tests.helpers import nv_f64_ref as ref
from tests.helpers import nv_shape_cases as sc

KNOBS = ("D2FE_NV_LEGACY", "D2FE_NV_PAIR", "D2FE_NV_XBLOCK", "D2FE_NV_BLOCKS", "D2FE_NV_TAIL_BLOCKS", "D2FE_NV_NBUF", "D2FE_NV_FRONT_TPW", "D2FE_NV_SLABSUM",
         "D2FE_NV_GROUP_RULE", "D2FE_NV_MERGE")


@pytest.fixture(scope="module")
def dev():
    from d2slam_amd import api, build
    build.build(dev=True)
    return api.DevFrontEnd


def _plan(dev, monkeypatch, case, size_i):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in case["env"].items():
        monkeypatch.setenv(k, v)
    arch, under = sc._arch(case, case["sizes"][size_i])
    plan = dev.netvlad_plan(arch, case["head"][1])
    assert [p[1] for p in plan] == [0] + [p[2] + 1 for p in plan[:-1]] and plan[-1][2] == len(arch) - 1      # every layer in exactly one step
    return plan, arch, under


@pytest.mark.parametrize("mult", [0.75, 0.35])
def test_reference_pinned_to_the_oracle(mult):
    """Every layer of the stand-in trunk, the pre-projection and the descriptor (with and without PCA): the float64 reference on the oracle's own input to
    that layer agrees with the oracle's fp32 result within the fp32 summation bound."""
    from d2slam_amd import netvlad as nvm
    from d2slam_amd.synth import synth_image
    from oracle import oracle as orc
    orc.build()
    nv = nvm.synthetic_netvlad_weights(seed=31, depth_multiplier=mult)
    img = synth_image(96, 128, 17)
    comp, mean = nvm.synthetic_netvlad_pca(96)
    desc, outs, feat, raw = orc.netvlad_forward(img, nv, pca=(comp, mean), return_layers=True)
    worst = 0.0
    for i, l in enumerate(nv["layers"]):
        x = img if i == 0 else outs[i - 1].astype(np.float64)
        r = ref.chain([l], x, res=outs[l["res"]].astype(np.float64) if l["res"] >= 0 else None)
        assert r["y"].shape == outs[i].shape
        q = ref.compare(outs[i], r["y"], r["bound"])
        assert q <= 1.0, (i, l["kind"], q)
        worst = max(worst, q)
    hd = nv["head"]
    r = ref.chain([dict(kind="pw", weight=hd["pre_w"], bias=hd["pre_b"], act=ref.ACT_NONE, stride=1)], outs[-1].astype(np.float64))
    assert ref.compare(feat, r["y"], r["bound"]) <= 1.0
    d, e, mass = ref.head(feat.reshape(-1, feat.shape[-1]).astype(np.float64), hd["assign_w"], hd["assign_b"], hd["centroids"], mfma=False)
    assert ref.compare(raw, d, e) <= 1.0
    assert abs(np.linalg.norm(d) - 1.0) < 1e-12
    y, ey = ref.pca(raw.astype(np.float64), np.zeros(raw.shape[0]), comp, mean)
    assert ref.compare(desc, y, ey) <= 1.0
    # and the chained float64 forward stays within the project's 1e-4 descriptor claim of the fp32 oracle
    d64, _, _ = ref.forward(img, nv)
    assert np.abs(d64 - raw).max() <= 1e-4


@pytest.mark.parametrize("case", sc.CASES, ids=[c["name"] for c in sc.CASES])
def test_case_is_planned_as_claimed(dev, monkeypatch, case):
    """the execution plan puts the step kind the case claims to test at its block(s) under test, at every image size of the case; a member the
    predicates refuse is planned as something else"""
    for si in range(len(case["sizes"])):
        plan, arch, under = _plan(dev, monkeypatch, case, si)
        assert under
        for u in under:
            hit = any(p[0] == case["kind"] and (p[1], p[2]) == u for p in plan)
            assert hit != case["refused"], (case["name"], si, u, plan)
        if case["family"] == "pblock2":
            assert [p[3] for p in plan if (p[1], p[2]) == under[0]] == [2]


def test_case_table_covers_every_compiled_shape(dev):
    """nv_pblock_kernel: the (NK, NT) the table's cases launch are exactly the compiled ones; the other families list every member of their products"""
    compiled = dev.netvlad_shapes(0)
    assert len(compiled) == len(set(compiled)) == 29
    got = set()
    for c in sc.CASES:
        if c["family"] in ("pblock", "pblock2"):
            b = c["block"]
            halves = [b["cout"]] if b["cout"] <= 128 else [(b["cout"] // 2 + 15) // 16 * 16, b["cout"] - (b["cout"] // 2 + 15) // 16 * 16]
            shapes = {(b["cin"] // 4, (h + 15) // 16) for h in halves}
            if c["family"] == "pblock":
                assert shapes == {c["member"]}
            got |= shapes
    assert got == set(compiled) == set(sc.PBLOCK_SHAPES)
    assert set(dev.netvlad_shapes(1)) == set(sc.MERGE_SHAPES) <= got
    for fam, members in sc.PRODUCTS.items():
        listed = [c["member"] for c in sc.CASES if c["family"] == fam]
        assert set(listed) == members and len(listed) == len(members), fam
        assert not any(c["refused"] for c in sc.CASES if c["family"] == fam)      # none of these members is refused; the refusals are cases of their own
    # what a member means in channels: the kernels' own tile / chunk functions
    for c in sc.CASES:
        b, m = c["block"], c["member"]
        if c["family"] == "fpair":
            assert ((c["first"][1] + 15) // 16, 2 if c["first"][0] > 16 else 1) == m
        elif c["family"] == "xblock":
            nj = 0 if b["cin"] == 8 else (b["cin"] + 15) // 16
            assert (b["stride"], nj, sc.block_ntiles(b["cout"])) == m
        elif c["family"] == "block" and b:
            assert sc.block_ntiles(b["cout"]) == m[1] and b["stride"] == int(m[0][-1]) and b["expand"] == m[0].startswith("expand")
        elif c["family"] == "block":
            assert sc.block_ntiles(c["first"][1] if m[0] == "front" else c["head"][1]) == m[1]
    assert [c for c in sc.CASES if c["refused"]], "the LDS refusal is a case of the table"


@pytest.mark.parametrize("family", sorted({c["family"] for c in sc.CASES}))
def test_inputs_exercise_both_clamps(family):
    """on the float64 reference of every case, at every size, at least 5 % of what enters each ReLU6 lies below 0 and at least 5 % above 6 (over the images
    the GPU test runs), so a missing clamp changes the result"""
    for case in [c for c in sc.CASES if c["family"] == family]:
        for si in range(len(case["sizes"])):
            net = sc.build_net(case, si)
            pre = [[] for _ in net["layers"]]
            for img in sc.images(case, si):
                outs, cur = [], img
                for li, l in enumerate(net["layers"]):
                    r = ref.chain([l], cur, res=outs[l["res"]] if l["res"] >= 0 else None)
                    pre[li].append(r["pre"][0].ravel()); outs.append(r["y"]); cur = r["y"]
            for li, l in enumerate(net["layers"]):
                if l["act"] != ref.ACT_RELU6:
                    continue
                z = np.concatenate(pre[li])
                lo, hi = float((z < 0).mean()), float((z > 6).mean())
                assert lo >= 0.05 and hi >= 0.05, (case["name"], si, li, lo, hi)


def _mutants(case, net, u, good):
    """the wrong kernels the comparator must reject at plan step u = (l0, l1) of this case's network (good: the reference of that step)"""
    layers = sc.step_layers(net, u)
    chid = layers[-1]["cin"]
    spatial = any(l["kind"] == "dw" for l in layers)
    # (a) ONE hidden channel left out of ONE 16-channel output tile: a channel of median activity among those the ReLU6 does not zero everywhere
    hidden = ref.act(good["pre"][-2], layers[-2]["act"]).reshape(-1, chid).mean(axis=0)
    live = np.flatnonzero(hidden > 0)
    c = int(live[np.argsort(hidden[live])[len(live) // 2]])
    tile = (layers[-1]["cout"] // 16) // 2
    M = {"a hidden channel left out": dict(skip_hidden=(c, slice(16 * tile, 16 * tile + 16))),
         "an output bias omitted": dict(skip_bias=int(np.argmax(np.abs(layers[-1]["bias"]))))}
    if len(layers) > 1:
        M["the first stage's upper clamp removed"] = dict(no_hi_clamp=True)
    if spatial:
        M["the (., +1) tap of the last column from the wrong column"] = dict(dw_wrong_tap=True)
        M["the last column of an odd-width map from its neighbour"] = dict(lastcol_from_neighbour=True)
    if chid // 16 >= 9:          # hidden channels in three or more groups: ceil(chunks / 4) chunks each (nv_groups)
        cpg = (chid // 16 + 3) // 4
        M["the slabs beyond the second not added"] = dict(only_hidden=slice(0, 2 * cpg * 16))
    return M


@pytest.mark.parametrize("family", sorted({c["family"] for c in sc.CASES}))
def test_comparator_rejects_mutants(family):
    """every block under test of every case, on the largest map of the case (odd width, several tiles): the unperturbed reference passes its own bound with
    fp32-rounded values, every mutant fails it"""
    seen = set()
    for case in [c for c in sc.CASES if c["family"] == family]:
        si = len(case["sizes"]) - 1
        net = sc.build_net(case, si)
        outs, cur = [], sc.images(case, si)[1]
        for l in net["layers"]:
            r = ref.chain([l], cur, res=outs[l["res"]] if l["res"] >= 0 else None)
            outs.append(r["y"]); cur = r["y"]
        for u in net["under"]:
            layers = sc.step_layers(net, u)
            x = sc.images(case, si)[1] if u[0] == 0 else outs[u[0] - 1]
            rl = layers[-1]["res"]
            res = outs[rl] if rl >= 0 else None
            good = ref.chain(layers, x, res=res)
            assert good["y"].shape[1] % 2 == 1 or not any(l["kind"] == "dw" for l in layers)
            assert ref.compare(good["y"].astype(np.float32), good["y"], good["bound"]) <= 1.0
            for name, mut in _mutants(case, net, u, good).items():
                bad = ref.chain(layers, x, res=res, mut=mut)
                assert ref.compare(bad["y"].astype(np.float32), good["y"], good["bound"]) > 1.0, (case["name"], u, name)
                seen.add(name)
    # all six where the block has them; the first block and a depthwise + project pair have no hidden-channel groups, the tail no depthwise stage
    assert len(seen) == {"fpair": 5, "refused": 5, "tail": 4}.get(family, 6), (family, seen)
