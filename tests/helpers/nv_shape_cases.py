"""The case table of tests/test_netvlad_shapes_cpu.py and tests/test_netvlad_shapes.py: one tiny network per compiled shape of the NetVLAD block kernels
(netvlad_pair.hip, netvlad_fused.hip), built so that the execution plan of d2fe_load_netvlad puts exactly that shape at the block under test.

A network is: first conv (16 / 24 / 32 channels) + first block -> the stride-2 blocks that shrink the map -> the block under test (repeated once with a
residual where Cin = Cout) -> a last 1x1 -> the head.  The image sizes put a map of at most 2 x 3, an odd x odd map inside one tile and an odd map of several
tiles with a partial last tile (13 x 23) at the block under test; a stride-2 block sees even and odd inputs in both dimensions (SAME pad_begin 0 and 1).

Weights: He-uniform, then every layer is rescaled on the float64 reference of the case's first image so that a fifth of what enters each ReLU6 lies above 6
(about half lies below 0) and every linear output has unit variance: both clamps of every fused block are active (the CPU test asserts the shares)."""
import numpy as np

from tests.helpers import nv_f64_ref as ref

# plan step kinds of d2fe_debug_netvlad_plan (include/d2fe_debug.h)
CONV0, DW, PW, FRONT, EXPAND, BLOCK, XBLOCK, PBLOCK, FPAIR, TAIL, TAIL_BLOCK = range(11)
FUSED_LINEAR = (FRONT, EXPAND, BLOCK, XBLOCK, PBLOCK, FPAIR)      # steps whose (linear) output may be written as partial slabs

# (NK = Cin / 4, NT) of nv_pblock_kernel as this table believes them compiled; the CPU test holds the set to d2fe_debug_netvlad_shapes
PBLOCK_SHAPES = [(2, 1), (2, 2), (2, 4), (2, 8), (4, 1), (4, 2), (4, 4), (4, 8), (6, 1), (6, 2), (6, 3), (6, 4), (6, 8), (8, 1), (8, 2), (8, 4), (8, 8),
                 (12, 3), (12, 4), (12, 5), (14, 1), (14, 2), (14, 4), (14, 7), (14, 8), (18, 5), (18, 8), (30, 7), (30, 8)]
MERGE_SHAPES = [(12, 3), (18, 5)]

# (H, W, first conv stride, stride-2 blocks before the block under test)
SIZES_S1 = [(32, 48, 2, 3), (34, 50, 2, 2), (50, 90, 2, 1)]          # the block under test sees 2 x 3, 5 x 7, 13 x 23
SIZES_S2 = [(32, 48, 2, 2), (34, 50, 2, 1), (52, 90, 1, 1)]          # ... 4 x 6, 9 x 13, 26 x 45 in; 2 x 3, 5 x 7, 13 x 23 out
SIZES_FIRST = [(32, 32, 2, 1), (33, 45, 2, 1), (33, 45, 1, 1)]       # the first block's own map: the API's minimum image, odd sizes, a first conv of stride 1
N_BATCH = 3


def pblock_cout(nk, nt):
    """output channels of the pixel-pair case (nk, nt): Cin where that fills nt tiles (then the block is repeated with a residual), else a partial last tile"""
    cin = 4 * nk
    return cin if (cin + 15) // 16 == nt else 16 * nt - 8


def block_ntiles(cout):
    """16-channel output tiles nv_block_kernel / nv_xblock_kernel are instantiated for (nv_block_ntiles)"""
    nt = (cout + 15) // 16
    return nt if nt <= 2 else 4 if nt <= 4 else 8


def _cases():
    C = []

    def add(family, member, kind, sizes, env=None, first=(16, 16), block=None, repeat=False, feat=64, head=(32, 128), refused=False, tail_cin=None, note=""):
        C.append(dict(family=family, member=member, kind=kind, sizes=sizes, env=dict(env or {}), first=first, block=block, repeat=repeat, feat=feat,
                      head=head, refused=refused, tail_cin=tail_cin, note=note, name="%s-%s" % (family, "-".join(str(m) for m in member)), index=len(C)))

    c0s = (16, 24, 32)
    # nv_pblock_kernel: every (NK, NT); chid 96 (two hidden-channel groups, summed by the consumer) and, in the repeated block, 192 (four, the slab-sum launch)
    for i, (nk, nt) in enumerate(PBLOCK_SHAPES):
        cin, cout = 4 * nk, pblock_cout(nk, nt)
        add("pblock", (nk, nt), PBLOCK, SIZES_S1, first=(c0s[i % 3], 16), block=dict(cin=cin, chid=96 if cin == cout else 192, cout=cout, stride=1, expand=True),
            repeat=cin == cout)
    # more than 128 output channels: two launches over channel halves (30, 8) + (30, 7)
    add("pblock2", (30, 8, 7), PBLOCK, SIZES_S1, block=dict(cin=120, chid=192, cout=240, stride=1, expand=True), feat=64)
    # nv_fpair_kernel: NT x NCH (one or two chunks of 16 first-conv channels)
    for nt in (1, 2, 4, 8):
        for nch, c0 in ((1, 16), (2, 24 if nt in (1, 4) else 32)):
            add("fpair", (nt, nch), FPAIR, SIZES_FIRST, first=(c0, 16 * nt - 8))
    # nv_xblock_kernel: stride 1 (the pixel-pair kernels off, or a width they do not have), stride 2
    for nj, cin in ((0, 8), (1, 16), (2, 32), (4, 64), (7, 112)):
        for nt in (1, 2, 4, 8):
            cout = cin if block_ntiles(cin) == nt else 16 * nt - 8
            add("xblock", (1, nj, nt), XBLOCK, SIZES_S1, env={"D2FE_NV_PAIR": "0"}, block=dict(cin=cin, chid=96 if cin == cout else 192, cout=cout, stride=1, expand=True),
                repeat=cin == cout)
    for nj, cin in ((0, 8), (1, 16), (2, 32)):
        for nt in (1, 2, 4, 8):
            add("xblock", (2, nj, nt), XBLOCK, SIZES_S2, block=dict(cin=cin, chid=192, cout=16 * nt - 8, stride=2, expand=True))
    # nv_xblock_kernel at widths that do not fill the NJ float4 loads of a lane group (zero rows beyond Cin in the expand record, masked loads in the kernel)
    add("xblockp", (1, 24), XBLOCK, SIZES_S1, env={"D2FE_NV_PAIR": "0"}, block=dict(cin=24, chid=96, cout=24, stride=1, expand=True), repeat=True)      # NJ 2
    add("xblockp", (1, 48), XBLOCK, SIZES_S1, env={"D2FE_NV_PAIR": "0"}, block=dict(cin=48, chid=96, cout=48, stride=1, expand=True), repeat=True)      # NJ 4
    add("xblockp", (1, 80), XBLOCK, SIZES_S1, block=dict(cin=80, chid=96, cout=80, stride=1, expand=True), repeat=True)                                 # NJ 7
    add("xblockp", (2, 24), XBLOCK, SIZES_S2, block=dict(cin=24, chid=192, cout=56, stride=2, expand=True))                                             # NJ 2
    # nv_block_kernel: expand and no-expand forms at both strides, the front form, the tail form
    for nt in (1, 2, 4, 8):
        cout = 16 * nt - 8
        add("block", ("expand1", nt), EXPAND, SIZES_S1, env={"D2FE_NV_PAIR": "0", "D2FE_NV_XBLOCK": "0"},
            block=dict(cin=24, chid=192, cout=24 if nt == 2 else cout, stride=1, expand=True), repeat=nt == 2)
        add("block", ("expand2", nt), EXPAND, SIZES_S2, env={"D2FE_NV_XBLOCK": "0"}, block=dict(cin=24, chid=192, cout=cout, stride=2, expand=True))
        add("block", ("noexpand1", nt), BLOCK, SIZES_S1, block=dict(cin=96, chid=96, cout=cout, stride=1, expand=False))
        # (stride 2 keeps a 17 x 33 input patch of every channel in LDS: 160 KB hold 48 channels beside the weights of 8 output tiles, not 96 -- a wider
        # depthwise + project pair is planned as two single layers)
        add("block", ("noexpand2", nt), BLOCK, SIZES_S2, block=dict(cin=48, chid=48, cout=cout, stride=2, expand=False))
        add("block", ("front", nt), FRONT, SIZES_FIRST, env={"D2FE_NV_PAIR": "0"}, first=(16 if nt in (1, 4) else 32, cout))
        # the last 1x1 (Cin 24: not one of nv_tail_kernel's) + a pre-projection of NT tiles; the head is then K x D with D = 16 NT (12 clusters: the general kernel)
        add("block", ("tail", nt), TAIL_BLOCK, SIZES_S1, block=None, first=(16, 16), feat=192, head=(32, 128) if nt == 8 else (12, 16 * nt), tail_cin=24)
    add("refused", ("noexpand2", 96), BLOCK, SIZES_S2, block=dict(cin=96, chid=96, cout=120, stride=2, expand=False), refused=True,
        note="160 KB of LDS do not hold the 17 x 33 x 96 input patch: nv_block_supported refuses, the pair runs as two single layers")
    # nv_tail_kernel
    for cin in (112, 128, 240):
        add("tail", (cin,), TAIL, SIZES_S1, feat=192, tail_cin=cin)
    return C


CASES = _cases()
PRODUCTS = {
    "fpair": {(nt, nch) for nt in (1, 2, 4, 8) for nch in (1, 2)},
    "xblock": {(1, nj, nt) for nj in (0, 1, 2, 4, 7) for nt in (1, 2, 4, 8)} | {(2, nj, nt) for nj in (0, 1, 2) for nt in (1, 2, 4, 8)},
    "block": {(f, nt) for f in ("expand1", "expand2", "noexpand1", "noexpand2", "front", "tail") for nt in (1, 2, 4, 8)},
    "tail": {(112,), (128,), (240,)},
}


def _he(rng, kind, cin, cout):
    if kind == "conv":
        fan, shape = 9, (cout, 1, 3, 3)
    elif kind == "dw":
        fan, shape = 9, (cin, 3, 3)
    else:
        fan, shape = cin, (cout, cin)
    b = np.sqrt(3.0 / fan)
    return rng.uniform(-b, b, size=shape).astype(np.float32), rng.uniform(-0.05, 0.05, size=(shape[0],)).astype(np.float32)


def _arch(case, size):
    """-> (layer dicts without weights, (l0, l1) of every block under test)"""
    H, W, s0, nshrink = size
    c0, first_out = case["first"]
    blk = case["block"]
    tail_cin = case.get("tail_cin")      # the last 1x1 itself is under test: its input width
    first_block = case["family"] == "fpair" or (case["family"] == "block" and case["member"][0] == "front")
    L, under = [], []

    def lay(kind, cin, cout, stride=1, a=ref.ACT_NONE, res=-1):
        L.append(dict(kind=kind, cin=cin, cout=cout, stride=stride, act=a, res=res))

    def block(cin, chid, cout, stride, expand, res=-1):
        l0 = len(L)
        if expand:
            lay("pw", cin, chid, a=ref.ACT_RELU6)
        lay("dw", chid, chid, stride, ref.ACT_RELU6)
        lay("pw", chid, cout, res=res)
        return (l0, len(L) - 1)

    lay("conv", 1, c0, s0, ref.ACT_RELU6)
    lay("dw", c0, c0, 1, ref.ACT_RELU6)
    lay("pw", c0, first_out)
    if first_block:
        under.append((0, 2))
    c = first_out
    want = blk["cin"] if blk else (tail_cin if tail_cin else 16)
    for i in range(nshrink):
        nxt = want if i == nshrink - 1 else 16
        block(c, 96, nxt, 2, True)
        c = nxt
    if blk:
        assert c == blk["cin"], (case["name"], c)
        under.append(block(c, blk["chid"], blk["cout"], blk["stride"], blk["expand"]))
        c = blk["cout"]
        if case["repeat"]:
            under.append(block(c, 192, c, 1, True, res=len(L) - 1))
    lay("pw", c, case["feat"], a=ref.ACT_RELU6)
    if tail_cin:
        under.append((len(L) - 1, len(L) - 1))
    return L, under


def images(case, size_i, n=N_BATCH):
    H, W = case["sizes"][size_i][:2]
    return np.random.RandomState(1000 + 7 * case["index"] + size_i).randint(0, 256, size=(n, H, W)).astype(np.uint8)


_NETS = {}


def build_net(case, size_i):
    """-> dict(layers, head, under, H, W): calibrated float32 weights (see the module docstring); cached"""
    key = (case["name"], case["index"], size_i, case["head"], case["sizes"][size_i])
    if key in _NETS:
        return _NETS[key]
    size = case["sizes"][size_i]
    arch, under = _arch(case, size)
    rng = np.random.RandomState(5000 + 13 * case["index"] + size_i)
    img = images(case, size_i)[0]
    outs, cur, layers = [], img, []
    for l in arch:
        w, b = _he(rng, l["kind"], l["cin"], l["cout"])
        l = dict(l, weight=w, bias=np.zeros_like(b))
        res = outs[l["res"]] if l["res"] >= 0 else None
        z = ref.chain([l], cur)["pre"][0]
        if l["act"] == ref.ACT_RELU6:
            q = float(np.quantile(z, 0.8))
            s = 6.0 / q if q > 1e-6 else 1.0
        else:
            s = 1.0 / max(float(z.std()), 1e-6)
        # biases of the size of the outputs (+-1 before a ReLU6 that spans 0..6, +-0.5 on a unit-variance linear output): a dropped bias is far beyond any rounding
        l["weight"] = (w * np.float32(s)).astype(np.float32); l["bias"] = (b * np.float32(20.0 if l["act"] == ref.ACT_RELU6 else 10.0)).astype(np.float32)
        y = ref.chain([l], cur, res=res)["y"]
        layers.append(l); outs.append(y); cur = y
    K, D = case["head"]
    feat = case["feat"]
    pre_w, pre_b = _he(rng, "pw", feat, D)
    z = cur @ pre_w.astype(np.float64).T
    pre_w = (pre_w / np.float32(max(float(z.std()), 1e-6))).astype(np.float32)
    head = dict(pre_w=pre_w, pre_b=(pre_b * np.float32(10.0)).astype(np.float32),
                assign_w=rng.normal(0, 1.0 / np.sqrt(D), size=(K, D)).astype(np.float32), assign_b=rng.uniform(-0.1, 0.1, size=(K,)).astype(np.float32),
                centroids=rng.normal(0, 0.3, size=(K, D)).astype(np.float32))
    net = dict(layers=layers, head=head, under=under, H=size[0], W=size[1])
    _NETS[key] = net
    return net


def pre_projection(net):
    """the NetVLAD pre-projection as a 1x1 layer"""
    hd = net["head"]
    return dict(kind="pw", cin=hd["pre_w"].shape[1], cout=hd["pre_w"].shape[0], stride=1, act=ref.ACT_NONE, res=-1, weight=hd["pre_w"], bias=hd["pre_b"])


def step_layers(net, u):
    """the layers plan step (l0, l1) evaluates: a step that ends with the trunk's last layer goes on through the pre-projection (the tail kernels, or the
    generic 1x1 launch behind an unfused last layer: either way the features are what can be read back)"""
    L = net["layers"][u[0]:u[1] + 1]
    return L + [pre_projection(net)] if u[1] == len(net["layers"]) - 1 else L


def out_slabs_max(layers, step):
    """upper limit of the partial slabs the output of plan step (kind, l0, l1, halves) is summed from (nv_plan: gmax of a fused step with a linear output;
    feat_gmax of the tail)"""
    kind, l0, l1 = step[:3]
    if kind in (TAIL, TAIL_BLOCK):
        return max(1, min(16, layers[l1]["cout"] // 32))
    if kind in FUSED_LINEAR and layers[l1]["act"] == ref.ACT_NONE:
        return max(1, min(16, layers[l1]["cin"] // 16 // 2))
    return 1
