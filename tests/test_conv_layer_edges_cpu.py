"""CPU half of tests/test_conv_layer_edges.py (no GPU): the inputs of tests/helpers/conv_layer_ref.py are what they claim to be, and the comparisons the GPU tests
make would notice a wrong kernel.

  1. every exact case is exact: the premise (sum |terms| below 2^24 units at every output) holds, and the int64, the float64 and a shuffled fp32 evaluation agree
     bit for bit;
  2. every case reaches what it names: the clamps act, ties round to both parities, subnormal operands decide the output, lo_x lo_w is not zero, the partial
     channel tiles and the walk lengths are the intended ones;
  3. the random-input cases satisfy the stated condition on the reference alone: the bound is at most 1 % of the tensor's largest |y|;
  4. MUTANTS lists, per precision, a defect of a kernel and the case whose comparison rejects it; each is evaluated and must be rejected, and the unmutated
     evaluation must pass the same comparison."""
import numpy as np
import pytest

from tests.helpers import conv_layer_ref as R
from tests.helpers import f16_oracle as fo

GEOMS = ((64, 3, 64), (128, 3, 128), (256, 1, 65))      # (Cin, k, Cout) of the exact cases: the three kernel geometries
EXACT = [(p, k, g) for p in (R.PREC_F16, R.PREC_F16X2) for k in R.EXACT_FOR[p] for g in GEOMS]


@pytest.mark.parametrize("prec,kind,geom", EXACT)
def test_exact_cases_are_exact(prec, kind, geom):
    x, w, b = R.exact_case(kind, *geom)
    ratio, q = R.exact_guard(prec, x, w, b)
    assert ratio < 1
    a = R.exact_value(prec, x, w, b, True, False, "int")
    assert R.same_bits(a, R.exact_value(prec, x, w, b, True, False, "f64"))
    assert R.same_bits(a, R.exact_value(prec, x, w, b, True, False, "f32shuffle"))
    assert (a > 0).mean() > 0.2      # the ReLU leaves outputs to compare ...
    pre = R.exact_value(prec, x, w, b, False, False, "int")
    assert (pre < 0).mean() > 0.02   # ... and cuts negative sums


@pytest.mark.parametrize("geom", GEOMS)
def test_exact_cases_reach_what_they_name(geom):
    # ties: 16 x and 256 w exactly between two fp16 neighbours, rounded to both parities (down and up)
    x, w, _ = R.exact_case("ties", *geom)
    for v, shift in ((x, R.SA), (w, R.SW)):
        s = np.abs(v.astype(np.float64) * 2.0 ** shift)
        h = np.abs(fo.round_operand(v, shift).astype(np.float64))
        tie = (s >= 2048) & (s % 2 == 1)
        assert tie.sum() > 15 and np.all(np.abs(h - s)[tie] == 1)
        assert (h[tie] < s[tie]).sum() > 4 and (h[tie] > s[tie]).sum() > 4
    # clamp: 4062.5, 5000, 1e9 and +inf all become 64992; weights beyond +-65000 / 256 become +-64992
    x, w, _ = R.exact_case("clamp", *geom)
    for val in (4062.5, 5000.0, 1e9, np.inf):
        assert (x == np.float32(val)).sum() > 0
    assert np.all(fo.round_operand(x[x >= 4062.5], R.SA).astype(np.float64) == 64992.0)
    big = np.abs(w) >= 65000.0 / 256
    assert big.sum() > 10 and (w[big] > 0).any() and (w[big] < 0).any() and (np.abs(w[big]) > 254).any()
    assert np.all(np.abs(fo.round_operand(w[big], R.SW).astype(np.float64)) == 64992.0)
    hi, lo = R.split16(x[x >= 4062.5], R.SA)
    assert np.all(hi.astype(np.float64) == 64992.0) and np.all(lo.astype(np.float64) == 8.0)      # F16X2: hi + lo = 65000, the clamp itself
    # subnormal: scaled operands k 2^-24 on both sides, and the output changes when they are flushed
    x, w, b = R.exact_case("subnormal", *geom)
    for v, shift in ((x, R.SA), (w, R.SW)):
        h = np.abs(fo.round_operand(v, shift).astype(np.float64))
        sub = (h > 0) & (h < 2.0 ** -14)
        assert sub.sum() > 50 and np.all(h[sub] == np.abs(v[sub].astype(np.float64)) * 2.0 ** shift)      # kept exactly
    keep = R.exact_value(R.PREC_F16, x, w, b, True, False)
    flushed = R.f16_layer(x, w, b, True, False, mutant="flush")[0]
    assert (keep != flushed.astype(np.float32)).mean() > 0.5
    # F16X2: the wide operands have a residual, and in wide_both the dropped product lo_x lo_w is not zero
    for kind, xs_wide, ws_wide in (("wide_x", True, False), ("wide_w", False, True), ("wide_both", True, True)):
        x, w, _ = R.exact_case(kind, *geom)
        (xh, xl), (wh, wl) = R.split16(x, R.SA), R.split16(w, R.SW)
        assert bool((xl != 0).any()) == xs_wide and bool((wl != 0).any()) == ws_wide
        assert np.array_equal(xh.astype(np.float64) + xl.astype(np.float64), x.astype(np.float64) * 2.0 ** R.SA)      # the split is exact on these grids
        assert np.array_equal(wh.astype(np.float64) + wl.astype(np.float64), w.astype(np.float64) * 2.0 ** R.SW)
    ll = R.corr(xl.astype(np.float64), wl.astype(np.float64))
    assert (ll != 0).mean() > 0.5


def test_sweep_tables_reach_what_they_name():
    for shape, couts in R.COUTS.items():
        bn = R.tile_of(2, shape)[2]
        assert couts[0] <= bn or shape == R.S1X1
        assert any(c % 32 for c in couts), "one cout leaves the last 32-channel tile partial"
        if shape != R.SFUSED:
            assert {-(-c // bn) for c in couts} >= {1, 2}, "one and two channel groups"
    for family in (1, 2):
        for shape, tile, pool, relu in R.compiled(family):
            th, tw, _ = R.tile_of(family, shape, tile)
            sizes = R.spatial_sizes(family, shape, tile)
            assert (2, 2) in sizes and (th, tw) in sizes and (th + 1, tw + 1) in sizes and (7, 47) in sizes
            assert any(h % 2 and w % 2 for h, w in sizes)      # under a pool the floor drops a row and a column
            tiles = [-(-h // th) * -(-w // tw) for h, w in sizes]
            assert 1 in tiles and max(tiles) >= 4
    assert len(R.compiled(1)) == 17 and len(R.compiled(2)) == 6
    # the walks: 3 images of 7x47
    n, H, W = R.WALK_GEOM
    for shape, cout, total in ((R.S64, 64, 12), (R.SFUSED, 64, 12), (R.S128_16, 256, 36), (R.S128_32, 128, 18), (R.S1X1, 256, 36)):
        assert R.pc_items(shape, n, H, W, cout) == total
        ncus = R.walk_ncus(total)
        grids = [min(total, c) for c in ncus]
        assert ncus[0] > total and grids[1] == total and total == grids[2] + 1 and grids[4] == 1
        assert -(-total // grids[3]) == 3 and total % grids[3]
    # conv1x1_256_65 with ncu = 1: two workgroups of four waves walk 31 m-tiles of 32 pixels in four rounds, the last pixel count no multiple of 32 or 128
    npix = n * H * W
    assert npix == 987 and npix % 32 and npix % 128 and min(-(-npix // 128), 2) == 2 and -(-(-(-npix // 32)) // 8) == 4


RANDOM = [(R.S64, 3, 7, 47, 128, True, True), (R.S128_32, 3, 7, 47, 256, True, True), (R.S128_16, 1, 5, 17, 128, False, True),
          (R.S1X1, 3, 7, 47, 256, False, False), (R.S1X1, 1, 2, 2, 65, False, False), (R.S64, 1, 2, 2, 64, False, True), (R.SFUSED, 3, 7, 47, 64, True, True)]


@pytest.mark.parametrize("prec", [R.PREC_F16, R.PREC_F16X2])
@pytest.mark.parametrize("case", RANDOM)
def test_random_cases_satisfy_the_stated_condition(orc, prec, case):
    shape, n, H, W, cout, pool, relu = case
    for ref in R.case_refs(prec, shape, n, H, W, cout, pool, relu):
        assert R.layer_limit_ok(ref), "bound %g against 1 %% of max |y| = %g" % (ref[2].max(), 0.01 * np.abs(ref[1]).max())


def test_f16_restatement_equals_the_f16_oracle():
    x, (w, b) = R.rand_act(1, 5, 33, 64)[0], R.rand_weights(64, 3, 64)
    y0, S0 = fo.layer(x, w, b, True, True)
    y1, S1 = R.f16_layer(x, w, b, True, True)
    assert np.abs(y0 - y1).max() <= 1e-12 * S0.max() and np.abs(S0 - S1).max() <= 1e-12 * S0.max()


# (precision, mutant, the case that rejects it).  Structural mutants: a random-input case of 5x33 pixels (odd: the pool's floor matters) with real numbers in the
# channels around the layer's own.  Operand and term mutants: only an EXACT case can see them.
STRUCT_CASE = "random 5x33, Cin 64 -> 64, ReLU, pool"
MUTANTS = [(p, m, STRUCT_CASE) for p in R.PRECS for m in R.STRUCT_MUTANTS] + [
    (R.PREC_F16, "trunc", "ties"), (R.PREC_F16, "noclamp", "clamp"), (R.PREC_F16, "flush", "subnormal"),
    (R.PREC_F16X2, "drop_hi_lo", "wide_w"), (R.PREC_F16X2, "drop_lo_hi", "wide_x"), (R.PREC_F16X2, "keep_lo_lo", "wide_both"), (R.PREC_F16X2, "trunc_hi", "wide_both")]
X2_MUT = {"drop_hi_lo": dict(terms=("hh", "lh")), "drop_lo_hi": dict(terms=("hh", "hl")), "keep_lo_lo": dict(terms=("hh", "hl", "lh", "ll")),
          "trunc_hi": dict(trunc_hi=True)}


@pytest.mark.parametrize("prec,mutant,case", MUTANTS)
def test_the_comparison_rejects_the_mutant(orc, prec, mutant, case):
    if case == STRUCT_CASE:
        H, W, cin, coff = 5, 33, 64, 8
        xfull = np.maximum(np.random.RandomState(3).randn(H, W, cin + 12), 0).astype(np.float32)
        w, b = R.rand_weights(cin, 3, 64)
        x = np.ascontiguousarray(xfull[:, :, coff:coff + cin])
        ref = R.reference(prec, orc, x, w, b, True, True)
        ok, _, txt = R.compare(R.evaluate(prec, orc, x, w, b, True, True), ref)
        assert ok, txt      # the unmutated evaluation passes
        mx, mw, mb, edge, anchor = R.mutant_inputs(mutant, xfull, coff, cin, w, b)
        ok, q, _ = R.compare(R.evaluate(prec, orc, mx, mw, mb, True, True, edge=edge, anchor_end=anchor), ref)
        assert not ok and (q is None or q > 4), "the comparison accepts %s" % mutant
        return
    for geom in GEOMS:
        x, w, b = R.exact_case(case, *geom)
        want = R.exact_value(prec, x, w, b, True, False)
        assert R.same_bits(R.evaluate(prec, orc, x, w, b, True, False), want)      # the unmutated evaluation passes
        kw = dict(mutant=mutant) if prec == R.PREC_F16 else X2_MUT[mutant]
        with np.errstate(invalid="ignore", over="ignore"):
            got = R.evaluate(prec, orc, x, w, b, True, False, **kw)
        assert not R.same_bits(got, want), "%s: the exact case %s accepts %s" % (geom, case, mutant)


@pytest.mark.parametrize("prec,mutant", [(R.PREC_F16X2, "drop_hi_lo"), (R.PREC_F16X2, "drop_lo_hi")])
def test_random_inputs_alone_would_accept_these_mutants(orc, prec, mutant):
    """why the exact cases exist: on random inputs a dropped cross term stays inside the summation bound"""
    x, (w, b) = R.rand_act(1, 5, 33, 128)[0], R.rand_weights(128, 3, 128)
    ref = R.reference(prec, orc, x, w, b, True, False)
    kw = dict(mutant=mutant) if prec == R.PREC_F16 else X2_MUT[mutant]
    ok, q, _ = R.compare(R.evaluate(prec, orc, x, w, b, True, False, **kw), ref)
    print("%s on random inputs: error / bound = %.3g" % (mutant, q))
    assert ok
