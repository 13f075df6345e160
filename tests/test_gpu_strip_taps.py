"""The strip kernel's 8-wave form (srh_strip.hip) reads the other view's rows 8 bytes at a time from ONE copy of the ring,
at candidate ranges that start on odd and on even columns, and its one-pass block loop takes the tap products
fma(w, l, -meanL)*w from an LDS plane built once per tile (block_onepass_taps, srh_block.hpp) instead of building them
in every block.  Neither changes a bit: `strip` = 8 is held here to `strip` = 0, the per-tile kernel, whose loop builds the
products inline.

  * cost rows (Context.twoview_cost_rows) over the whole image -- the rows the top and bottom edge cut included: they go
    through the border instantiation, whose row reads changed too -- in forms 0, 3 and 5, form 5 raw and with the redo,
    both directions, byte for byte;
  * the depth maps of twoview_wta and twoview_compute_device under the default arithmetic and `arith` 0: the same bits
    from both kernels, and the oracle's maps (1e-9 relative: the device exp differs from libm's).

Shapes (tests/small_shapes.py): 65 x 12 x 8 geodesic radius 5 (65 is no multiple of 32: the last tile is partial) and
33 x 9 x 40 adaptive radius 2 (ranges longer than one round of 128 columns), each plain and with masks; and 65 x 30 x 8
geodesic radius 5, whose 19 interior rows are one 8-row and three shorter work items: the plane is rewritten tile after
tile inside an item.

The per-tile kernel has no redo of its own (its uncertified candidates stay NaN for the scan).  Where it leaves none --
every case here, printed per fetch -- the redo rows are compared byte for byte like the others; were there one, the strip
kernel's entry would have to hold the bits of form 0 wherever it differs."""
import functools
import types

import numpy as np
import pytest

import cases
import oracle_ffi as O
import small_shapes as SS
from stereoreconstruction_amd import capi

pytestmark = pytest.mark.gpu

DIRECTIONS = ((0, 1), (1, 0))
UNWRITTEN = np.uint64(0xFFFFFFFFFFFFFFFF)
# (shape, radius, weight kind, masks)
TAP_CASES = [((65, 12, 8), 5, 1, False), ((65, 12, 8), 5, 1, True), ((33, 9, 40), 2, 0, False), ((33, 9, 40), 2, 0, True),
             ((65, 30, 8), 5, 1, False)]
IDS = ["%s_r%d_%s_%s" % (SS.shape_id(s), r, "geodesic" if k else "adaptive", "masks" if m else "plain") for s, r, k, m in TAP_CASES]
# (form, raw)
FETCHES = ((0, False), (3, False), (5, True), (5, False))


@functools.lru_cache(maxsize=None)
def _case(shape, radius, kind, masks):
    case = SS.small_twoview(*shape, radius, kind, masks=masks)
    imgs, ocams, op = cases.oracle_inputs(case)
    cams, p = cases.hip_inputs(case)
    return types.SimpleNamespace(case=case, imgs=imgs, ocams=ocams, op=op, cams=cams, p=p, w=shape[0], h=shape[1], tag=case["name"])


@functools.lru_cache(maxsize=None)
def _oracle(shape, radius, kind, masks):
    """the CPU oracle's two passes and their cross-check: computed once, shared, never written to"""
    c = _case(shape, radius, kind, masks)
    dl = O.twoview_wta(c.imgs[0], c.imgs[1], c.ocams[0], c.ocams[1], c.op)
    dr = O.twoview_wta(c.imgs[1], c.imgs[0], c.ocams[1], c.ocams[0], c.op)
    cl, cr = O.twoview_cross_check(c.ocams[0], c.ocams[1], c.op, dl, dr)
    for a in (dl, dr, cl, cr):
        a.setflags(write=False)
    return (dl, dr), (cl, cr)


def _rows(ctx, c, strip):
    """{(direction, form, raw): (cost, range)} under option strip"""
    out = {}
    ctx.set_option("strip", strip)
    try:
        for ref, oth in DIRECTIONS:
            for form, raw in FETCHES:
                cost, rng, us = ctx.twoview_cost_rows(ref, oth, c.p, 0, c.h, form, raw=raw)
                assert us == (strip != 0), "%s strip=%d: which kernel ran" % (c.tag, strip)
                out[(ref, form, raw)] = (cost, rng)
    finally:
        ctx.set_option("strip", 1)
    return out


@pytest.mark.parametrize("shape,radius,kind,masks", TAP_CASES, ids=IDS)
def test_cost_rows_have_the_per_tile_kernels_bits(hip_ctx, shape, radius, kind, masks):
    c = _case(shape, radius, kind, masks)
    cases.upload_case(hip_ctx, c.case, c.cams)
    tile, strip = _rows(hip_ctx, c, 0), _rows(hip_ctx, c, 8)
    n_live = 0
    for ref, _ in DIRECTIONS:
        exact0 = tile[(ref, 0, False)][0].view(np.uint64)
        for form, raw in FETCHES:
            tag = "%s ref %d form %d%s" % (c.tag, ref, form, " raw" if raw else "")
            (c0, r0), (c8, r8) = tile[(ref, form, raw)], strip[(ref, form, raw)]
            assert np.array_equal(r0, r8), tag
            b0, b8 = c0.view(np.uint64), c8.view(np.uint64)
            k = np.arange(c0.shape[2], dtype=np.int32)[None, None, :]
            live = (k <= (r0[..., 1] - r0[..., 0])[..., None]) & (b0 != UNWRITTEN)
            # what the per-tile kernel left uncertified; with the redo the strip kernel re-evaluates the candidate's whole
            # block in the reference's arithmetic, the per-tile kernel leaves the NaN to the scan
            unc = live & np.isnan(c0) if form != 0 else np.zeros_like(live)
            differ = b0 != b8
            print("%s: %d live entries, %d uncertified under strip = 0, %d differ" % (tag, live.sum(), unc.sum(), differ.sum()))
            n_live += int(live.sum())
            if raw or form == 0 or not unc.any():
                assert np.array_equal(b0, b8), "%s: %d entries differ, first (y, x, k) %s" % (tag, differ.sum(), [int(a[0]) for a in np.nonzero(differ)])
            else:
                assert not (differ & ~live).any(), tag
                assert np.array_equal(b8[differ], exact0[differ]), "%s: a redone entry is not the reference's" % tag
                assert np.array_equal(b8[unc], exact0[unc]), "%s: an uncertified candidate was not redone" % tag
    assert n_live > 0, c.tag


def _maps(ctx, c, strip, arith):
    """[twoview_wta 0>1, twoview_wta 1>0, twoview_compute_device left, right] under options strip and arith"""
    ctx.set_option("strip", strip)
    ctx.set_option("arith", arith)
    out = []
    try:
        for ref, oth in DIRECTIONS:
            ctx.twoview_wta(ref, oth, c.p)
            assert ctx.stats()["used_strip_kernel"] == (strip != 0), "%s strip=%d: which kernel ran" % (c.tag, strip)
            out.append(ctx.download_depth(ref))
        ctx.twoview_compute_device(0, 1, c.p)
        out += [ctx.download_depth(0), ctx.download_depth(1)]
    finally:
        ctx.set_option("strip", 1)
        ctx.set_option("arith", capi.ARITH_DEFAULT)
    return out


@pytest.mark.parametrize("shape,radius,kind,masks", TAP_CASES, ids=IDS)
def test_depth_maps_match_the_per_tile_kernel_and_the_oracle(hip_ctx, shape, radius, kind, masks):
    c = _case(shape, radius, kind, masks)
    wta, crossed = _oracle(shape, radius, kind, masks)
    want = list(wta) + list(crossed)
    names = ("wta 0>1", "wta 1>0", "compute left", "compute right")
    cases.upload_case(hip_ctx, c.case, c.cams)
    ref = _maps(hip_ctx, c, 0, 0)
    for strip, arith in ((8, capi.ARITH_DEFAULT), (8, 0), (0, capi.ARITH_DEFAULT)):
        got = _maps(hip_ctx, c, strip, arith)
        for g, r, name in zip(got, ref, names):
            assert np.array_equal(g.view(np.uint64), r.view(np.uint64)), \
                "%s strip=%d arith=%d %s: depth bits differ from the per-tile kernel in the reference's arithmetic" % (c.tag, strip, arith, name)
        if strip == 8:
            for g, w, name in zip(got, want, names):
                ok, msg, _ = cases.compare_depth(g, w, 1e-9)
                assert ok, "%s strip=8 arith=%d %s: %s" % (c.tag, arith, name, msg)
    print("%s: finite %d / %d" % (c.tag, np.isfinite(ref[0]).sum(), ref[0].size))
