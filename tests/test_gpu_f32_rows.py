"""The cost rows of the two cost kernels no other test looks into, entry by entry.

A. The single-precision kernel (srh_dense_f32.hip, option "arith" = 2, both "f32_form"s), fetched through
   srh_twoview_cost_rows(form = 2), against its CPU restatement tests/f32_restatement.cpp (pinned on the CPU by
   tests/test_f32_restatement_host.py).  The library is built without contraction, its float division and square root are
   correctly rounded, denormals are kept and every multiply-add of the block loops is an explicit fma: float, fmaf, / and
   sqrtf in the kernel's order are the kernel's exact image.  So, per case, direction and form:
     * ranges and the set of written entries are those of the reference's arithmetic (form 0); never the strip kernel;
     * every live entry of a STABLE pixel holds the restatement's bits.  (Stable: every weight, +- 8 ulp, and each pixel
       constant, +- 2^-40 relative, rounds to one float -- the device's exp differs from libm's by an ulp and its windows
       kernels sum the constants in other orders; decided on the CPU from the oracle's doubles.)  One class differs:
       the columns dense_cover_hi leaves out of the cost kernel, which twoview_lazy_fill_kernel writes in the reference's
       arithmetic: they hold form 0's bits and may only be among the last two columns of a pixel's range;
     * every live fast-form entry, stable or not, is within 2 B of the cost in double (B: the first-order bound of the
       restatement); unstable pixels are held to this only.
   Printed per case and form: entries compared bit for bit, unstable pixels, lazily filled entries, worst ratio to B.
   A mismatch is reported in the coordinates a kernel slip shows up in: tile column, position in the block of 8 from
   lo & ~3, position in the 320-column chunk, the path the restatement took.

B. The unchecked fused mode ("arith" = 1, cost-row form 1) against the certified two-sweep form 3 fetched raw, on the
   per-tile kernel and on the 4- and 8-wave strip kernels (test_fused_unchecked_rows_are_the_certified_sweeps)."""
import functools
import types

import numpy as np
import pytest

import cases
import f32_ref as F
import test_gpu_arith_modes as am
from stereoreconstruction_amd import capi, synthetic

pytestmark = pytest.mark.gpu

UNWRITTEN = np.uint64(0xFFFFFFFFFFFFFFFF)
CHUNK, TILE = 320, 32
# cost rows have to fit one band: the library's default budget, whatever halvings an earlier test's refused allocations left
# on the shared context (setting the option forgets them)
DEFAULT_BUDGET_MB = 32768
PATHS = {0: "none", F.FAST: "fast", F.GENERAL: "general"}

# (name, overrides, directions, wide): the smallest shapes at which each mechanism of the kernel exists
#   96x16 r = 5: the fast form on rows 5 .. 9, everything else the general path (s_need_pix / s_need_col, the glist rounds)
#   r = 2 at widths 31 / 32 / 33 / 65: the tile edge, lanes with x >= W, NRF = 12 with no slack
#   masks: reference pixels without a range, unusable taps on either side, lall = 0 pixels
#   400 wide, 300 labels: a tile's ranges span more than one chunk (blocks that straddle the chunk edge, rt restaged); near the
#   side borders the clipped ranges take every width, so dense_cover_hi leaves columns to the lazy fill
BOTH, ONE = ((0, 1), (1, 0)), ((0, 1),)
CASES = [("geodesic_rect", dict(w=96, h=16, D=24), BOTH, False),
         ("adaptive_rect", dict(w=96, h=16, D=24), BOTH, False),
         ("geodesic_r2", dict(w=31, h=9, D=24), BOTH, False),
         ("geodesic_r2", dict(w=32, h=9, D=24), BOTH, False),
         ("geodesic_r2", dict(w=33, h=9, D=24), BOTH, False),
         ("geodesic_r2", dict(w=65, h=9, D=24), BOTH, False),
         ("geodesic_masks", dict(w=70, h=20, D=20), BOTH, False),
         ("adaptive_masks", dict(w=70, h=20, D=20), BOTH, False),
         ("geodesic_rect", dict(w=400, h=14, D=300), ONE, True),
         ("geodesic_rect", dict(w=400, h=8, D=300, radius=2), ONE, True)]
IDS = ["%s_%dx%dx%d%s" % (n, o["w"], o["h"], o["D"], "_r2" if o.get("radius") == 2 else "") for n, o, _, _ in CASES]


def _valid(rng, cstride):
    """mask (rows, w, cstride): entry k of a pixel is a column of its range (test_gpu_cert_rows._valid)"""
    lo, hi = rng[..., 0], rng[..., 1]
    k = np.arange(cstride, dtype=np.int32)[None, None, :]
    return k <= (hi - lo)[..., None]


@functools.lru_cache(maxsize=None)
def _case(name, over):
    case = cases.get_twoview(name, **dict(over))
    imgs, _, op = cases.oracle_inputs(case)
    cams, p = cases.hip_inputs(case)
    return types.SimpleNamespace(case=case, imgs=imgs, op=op, cams=cams, p=p)


_RESTATED = {}


def _restated(name, over, ref, rng, cstride):
    """the restatement of one direction of a case over the device's column ranges: computed once, shared, never written to"""
    key = (name, over, ref)
    if key not in _RESTATED:
        c = _case(name, over)
        _RESTATED[key] = (rng.copy(), F.rows(c.imgs[ref], c.imgs[1 - ref], c.op, 0, c.imgs[ref].h, rng, cstride))
    rng0, r = _RESTATED[key]
    assert np.array_equal(rng0, rng), "the column ranges changed between two calls"
    return r


def _tile_cmin(rng):
    """(rows, w): the first chunk's start of the pixel's tile, (min lo of the tile's pixels with a range) & ~3 -- and the
    tile's largest hi"""
    rows, w, _ = rng.shape
    lo, hi = rng[..., 0].astype(np.int64), rng[..., 1].astype(np.int64)
    has = hi >= lo
    cmin, cmax = np.zeros((rows, w), np.int64), np.full((rows, w), -1, np.int64)
    for x0 in range(0, w, TILE):
        s = slice(x0, min(w, x0 + TILE))
        m = np.where(has[:, s], lo[:, s], np.iinfo(np.int64).max).min(axis=1) & ~3
        cmin[:, s] = m[:, None]
        cmax[:, s] = np.where(has[:, s], hi[:, s], -1).max(axis=1)[:, None]
    return cmin, cmax


def _where(bad, rng, cmin, r, got, want, n=6):
    """the first mismatches in the kernel's coordinates"""
    out = []
    for y, x, k in np.argwhere(bad)[:n]:
        lo = int(rng[y, x, 0])
        c = lo + int(k)
        out.append("(y %d, x %d, column %d): tile column %d, block position %d, chunk %d + %d, k %d of %d, path %s: got %r want %r"
                   % (y, x, c, x % TILE, (c - (lo & ~3)) % 8, (c - cmin[y, x]) // CHUNK, (c - cmin[y, x]) % CHUNK, k,
                      int(rng[y, x, 1]) - lo, PATHS[int(r.path[y, x, k])], got[y, x, k], want[y, x, k]))
    return "%d entries; %s" % (bad.sum(), "; ".join(out))


@pytest.mark.parametrize("name,over,directions,wide", CASES, ids=IDS)
def test_f32_cost_rows_hold_the_restatements_bits(hip_ctx, name, over, directions, wide):
    okey = tuple(sorted(over.items()))
    c = _case(name, okey)
    cases.upload_case(hip_ctx, c.case, c.cams)
    h = c.imgs[0].h
    mcd = c.p.max_color_diff
    n_lazy_seen, span_seen, n_edge = 0, 0, 0
    hip_ctx.set_option("band_budget_mb", DEFAULT_BUDGET_MB)
    try:
        for ref, oth in directions:
            hip_ctx.set_option("strip", 0)                     # the reference's arithmetic on the per-tile kernel: the same blocks
            exact, rng, us = hip_ctx.twoview_cost_rows(ref, oth, c.p, 0, h, 0)
            assert not us
            cstride = exact.shape[2]
            valid = _valid(rng, cstride)
            eb = exact.view(np.uint64)
            live = valid & (eb != UNWRITTEN)
            r = _restated(name, okey, ref, rng, cstride)
            assert np.array_equal(r.path != 0, valid)
            cmin, cmax = _tile_cmin(rng)
            has = rng[..., 1] >= rng[..., 0]
            # (dense_cover_hi trims at most two columns of a range: what is left of the widest tile union)
            span_seen = max(span_seen, int((cmax - 2 - cmin + 1)[has].max()))
            # live entries in the last column of a tile's first chunk and the first column of its second
            pos = rng[..., 0].astype(np.int64)[..., None] + np.arange(cstride)[None, None, :] - cmin[..., None]
            n_edge += int((live & ((pos == CHUNK - 1) | (pos == CHUNK))).sum())
            ranged = has.sum()
            unstable = has & ~r.stable
            assert unstable.sum() <= 0.01 * ranged, "%s %d>%d: %d of %d pixels unstable: a bad input" % (name, ref, oth, unstable.sum(), ranged)
            k = np.arange(cstride)[None, None, :]
            last_two = k >= (rng[..., 1] - rng[..., 0] - 1)[..., None]
            for form in (0, 1):
                tag = "%s %s %d>%d f32_form %d" % (name, over, ref, oth, form)
                hip_ctx.set_option("f32_form", form)
                for strip in (1, 8):
                    hip_ctx.set_option("strip", strip)
                    got, rng2, us = hip_ctx.twoview_cost_rows(ref, oth, c.p, 0, h, 2)
                    assert not us, "%s: the f32 rows came from the strip kernel (strip = %d)" % (tag, strip)
                    assert got.shape == exact.shape and np.array_equal(rng, rng2), tag
                    if strip == 1:
                        first = got
                    else:
                        assert np.array_equal(first.view(np.uint64), got.view(np.uint64)), "%s: option strip changes the f32 rows" % tag
                got = first
                gb = got.view(np.uint64)
                assert np.array_equal(gb[valid] == UNWRITTEN, eb[valid] == UNWRITTEN), "%s: another set of entries is written" % tag
                want = r.f32[form]
                wb = want.view(np.uint64)
                stab = live & r.stable[..., None]
                differ = stab & (gb != wb)
                # the lazily filled columns: the reference's arithmetic, and only at the end of a range
                lazy = differ & (gb == eb) & last_two
                bad = differ & ~lazy
                assert not bad.any(), "%s: %s" % (tag, _where(bad, rng, cmin, r, got, want))
                n_lazy_seen += int(lazy.sum())
                # every fast-form entry against the cost in double
                fast = live & (r.path == F.FAST) & ~lazy
                out = fast & r.noB[form]
                chk = fast & ~r.noB[form]
                assert out.sum() <= 0.01 * max(1, fast.sum()), "%s: %d of %d fast-form entries have no first-order bound" % (tag, out.sum(), fast.sum())
                d = np.abs(got[chk] - r.f64[chk])
                ratio_all = np.zeros(got.shape)
                ratio_all[chk] = d / r.B[form][chk]
                worst = float(ratio_all.max())
                print("f32 rows %s: %d entries compared bit for bit, %d unstable pixels of %d (their %d entries within 2 B only), "
                      "%d lazily filled entries hold the reference's bits, %d fast-form entries: max |f32 - f64| = %.3g, worst |f32 - f64| / B = %.3g"
                      % (tag, stab.sum(), unstable.sum(), ranged, (live & ~r.stable[..., None]).sum(), lazy.sum(), chk.sum(),
                         d.max() if d.size else 0.0, worst))
                assert not np.isnan(d).any(), tag
                toofar = chk & ~(ratio_all <= 2.0)
                assert not toofar.any(), "%s: beyond 2 B: %s" % (tag, _where(toofar, rng, cmin, r, got, r.f64))
                assert stab.sum() > 0 and (got[live] <= max(mcd, c.p.bad_ret)).all()
    finally:
        hip_ctx.set_option("f32_form", 0)
        hip_ctx.set_option("strip", 1)
    if wide:
        # both situations the wide cases exist for, from the returned ranges and rows alone
        assert span_seen > CHUNK, "%s: no tile's ranges span more than one chunk (%d columns)" % (name, span_seen)
        assert n_edge > 0, "%s: no live entry on either side of a chunk edge" % name
        assert n_lazy_seen > 0, "%s: no entry that holds the reference's bits and not the restatement's: the lazy fill was not reached" % name


@pytest.mark.parametrize("name,over", am.CERT_CASES)
@pytest.mark.parametrize("strip", [0, 4, 8])
def test_fused_unchecked_rows_are_the_certified_sweeps(hip_ctx, name, over, strip):
    """Cost-row form 1 ("arith" = 1: fused multiply-adds, no certificate) against form 3 fetched raw (the certified two fused
    sweeps without the in-kernel redo).  In the per-tile kernel (twoview_dense_cost_kernel, FMA = AR != 0) AND in the strip
    kernel (two_sweeps<FMA, CERT> of twoview_strip_cost_kernel) both forms run ONE loop body, every multiply-add an explicit
    fma, and differ in the storing rule only -- so the bits are held on all three kernels, not a tolerance:
      * form 3 holds a number below max_color_diff: form 1 holds the same bits;
      * form 3 holds a number in [max_color_diff, max_color_diff + e0] (it keeps values up to its m_hi for the certified
        scan) or the clamp: form 1 holds the clamp;
      * form 3 holds a number beyond max_color_diff + e0: that is bad_ret out of the select forms, which both forms
        evaluate in the reference's arithmetic: the same bits (as tests/test_gpu_cert_rows.py reads such values);
      * form 3 holds NaN (not certified): form 1 holds a number, not NaN, at most the clamp."""
    case = cases.get_twoview(name, **over)
    cams, p = cases.hip_inputs(case)
    cases.upload_case(hip_ctx, case, cams)
    h = case["views"][0][0].shape[0]
    hip_ctx.set_option("band_budget_mb", DEFAULT_BUDGET_MB)
    hip_ctx.set_option("strip", strip)
    try:
        for ref, oth in ((0, 1), (1, 0)):
            n = _fused_rules(hip_ctx, p, ref, oth, h, strip, "%s %s strip=%d" % (name, over, strip))
            assert n[0] > 0
    finally:
        hip_ctx.set_option("strip", 1)


def _fused_rules(ctx, p, ref, oth, h, strip, tag):
    """form 1 against form 3 raw under the option strip already set -> the number of entries under each of the four rules"""
    cb = capi.cert_bound(p)
    assert cb["ok"]
    e0, mcd = cb["e0"], p.max_color_diff
    f3, rng, us3 = ctx.twoview_cost_rows(ref, oth, p, 0, h, 3, raw=True)
    f1, rng1, us1 = ctx.twoview_cost_rows(ref, oth, p, 0, h, 1)
    assert us1 == us3 == (strip != 0) and np.array_equal(rng, rng1), tag
    valid = _valid(rng, f3.shape[2])
    b3, b1 = f3.view(np.uint64), f1.view(np.uint64)
    assert np.array_equal(b3[valid] == UNWRITTEN, b1[valid] == UNWRITTEN), tag
    live = valid & (b3 != UNWRITTEN)
    unc = live & np.isnan(f3)
    with np.errstate(invalid="ignore"):
        below = live & (f3 < mcd)
        clamp = live & (f3 >= mcd) & (f3 <= mcd + e0)
        beyond = live & (f3 > mcd + e0)
    assert (unc | below | clamp | beyond)[live].all()
    cmin, _ = _tile_cmin(rng)
    r = types.SimpleNamespace(path=np.zeros(f3.shape, np.uint8))
    bad = (below | beyond) & (b1 != b3)
    assert not bad.any(), "%s %d>%d: form 1 is not form 3's bits: %s" % (tag, ref, oth, _where(bad, rng, cmin, r, f1, f3))
    bad = clamp & (f1 != mcd)
    assert not bad.any(), "%s %d>%d: form 1 is not the clamp: %s" % (tag, ref, oth, _where(bad, rng, cmin, r, f1, f3))
    bad = unc & ~(f1 <= mcd)
    assert not bad.any(), "%s %d>%d: an uncertified candidate: %s" % (tag, ref, oth, _where(bad, rng, cmin, r, f1, f3))
    n = (int(below.sum()), int(clamp.sum()), int(beyond.sum()), int(unc.sum()))
    print("fused rows %s %d>%d: %d entries hold form 3's bits, %d clamps, %d beyond the clamp, %d not certified by form 3" % ((tag, ref, oth) + n))
    return n


@pytest.mark.parametrize("strip", [0, 8], ids=["per-tile", "strip"])
@pytest.mark.parametrize("kind", ["flat", "near_flat", "saturated_half"])
def test_fused_unchecked_rows_where_the_certificate_fails(hip_ctx, kind, strip):
    """The same rules on images built to sit on them (test_gpu_arith_modes._adversarial_pair): flat and saturated windows
    are what form 3 does not certify (NaN) or stores as the clamp; the parity cases above hold neither."""
    W, H, D = 192, 96, 40
    L, R, ml, mr = am._adversarial_pair(kind, W, H, D)
    (Kl, Rl, tl), (Kr, Rr, tr) = synthetic.rectified_cameras(W, H)
    zmin, zmax = synthetic.rectified_depth_range(W, D)
    hip_ctx.upload_view(0, L, ml, capi.camera_from_krt(Kl, Rl, tl))
    hip_ctx.upload_view(1, R, mr, capi.camera_from_krt(Kr, Rr, tr))
    p = capi.params_twoview(min_depth=zmin, max_depth=zmax, num_depth_levels=D, weight_kind=capi.WEIGHT_GEODESIC)
    hip_ctx.set_option("band_budget_mb", DEFAULT_BUDGET_MB)
    hip_ctx.set_option("strip", strip)
    try:
        n = _fused_rules(hip_ctx, p, 0, 1, H, strip, "%s strip=%d" % (kind, strip))
    finally:
        hip_ctx.set_option("strip", 1)
    if kind == "flat":
        assert n[1] + n[3] > 0, "a flat pair with neither a clamp nor an uncertified candidate"


def test_cost_row_forms_that_do_not_exist(hip_ctx):
    """form 2 joined 0, 1, 3 and 5; anything else is still refused"""
    c = _case("geodesic_r2", tuple(sorted(dict(w=33, h=9, D=24).items())))
    cases.upload_case(hip_ctx, c.case, c.cams)
    for form in (-1, 4, 6):
        with pytest.raises(capi.StereoHipError):
            hip_ctx.twoview_cost_rows(0, 1, c.p, 0, 9, form)
