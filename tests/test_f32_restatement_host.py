"""tests/f32_restatement.cpp on the CPU, before any device is involved: the float restatement of the single-precision cost
kernel (srh_dense_f32.hip) against the same cost in double, within twice its own first-order forward error bound B
(derived in the .cpp; u = 2^-24; the factor 2 pays for the second-order terms the derivation drops -- nothing is fitted).

Per case, direction and form:
  * every fast-form entry: |f32 - f64| <= 2 B; an entry whose |d s3| > s3 / 4 has no first-order bound and is left out of
    this check only, at most 1 % of a case's fast-form entries;
  * every general-path entry (the select form in double on inputs rounded to float): within 1e-4 of f64;
  * at most 1 % of the pixels are unstable (an input within a few ulp of a float rounding boundary): more is a bad input;
  * the storing rule on hand-built windows: a NaN v stores the clamp.

tests/test_gpu_f32_rows.py holds the kernel's cost rows to this restatement bit for bit."""
import functools

import numpy as np
import pytest

import cases
import f32_ref as F

CASES = [("geodesic_rect", dict(w=96, h=16, D=24)), ("adaptive_rect", dict(w=96, h=16, D=24)), ("geodesic_r2", dict(w=97, h=9, D=24))]
IDS = ["%s_%dx%dx%d" % (n, o["w"], o["h"], o["D"]) for n, o in CASES]


@functools.lru_cache(maxsize=None)
def _rows(name, over, ref):
    case = cases.get_twoview(name, **dict(over))
    imgs, _, op = cases.oracle_inputs(case)
    rng, cstride = F.disparity_ranges(case, ref)
    return F.rows(imgs[ref], imgs[1 - ref], op, 0, imgs[ref].h, rng, cstride), op


def check_bound(r, form, tag):
    """the fast-form entries of r against f64 within 2 B -> (entries checked, left out, worst ratio to B)"""
    fast = r.path == F.FAST
    out = fast & r.noB[form]
    chk = fast & ~r.noB[form]
    assert out.sum() <= 0.01 * fast.sum(), "%s: %d of %d fast-form entries have no first-order bound" % (tag, out.sum(), fast.sum())
    d = np.abs(r.f32[form][chk] - r.f64[chk])
    B = r.B[form][chk]
    assert np.isfinite(B).all() and not np.isnan(d).any(), tag
    ratio = float((d / B).max()) if d.size else 0.0
    print("%s form %d: %d fast-form entries, %d left out, max |f32 - f64| = %.3g, max B = %.3g, worst |f32 - f64| / B = %.3g"
          % (tag, form, chk.sum(), out.sum(), d.max() if d.size else 0.0, B.max() if B.size else 0.0, ratio))
    assert ratio <= 2.0, "%s form %d: |f32 - f64| = %.3g B" % (tag, form, ratio)
    return int(chk.sum()), int(out.sum()), ratio


@pytest.mark.parametrize("ref", [0, 1], ids=["0>1", "1>0"])
@pytest.mark.parametrize("name,over", CASES, ids=IDS)
def test_restatement_against_the_double_cost(name, over, ref):
    r, op = _rows(name, tuple(sorted(over.items())), ref)
    tag = "%s %d>%d" % (name, ref, 1 - ref)
    fast, gen = r.path == F.FAST, r.path == F.GENERAL
    assert fast.sum() > 1000 and gen.sum() > 1000, (tag, fast.sum(), gen.sum())
    for form in (0, 1):
        n, _, _ = check_bound(r, form, tag)
        assert n > 0
        # the general path does not depend on the form
        assert np.array_equal(r.f32[0][gen], r.f32[1][gen])
    dg = np.abs(r.f32[0][gen] - r.f64[gen])
    assert not np.isnan(dg).any() and dg.max() <= 1e-4, "%s: general path %.3g from the double cost" % (tag, dg.max())
    ranged = (r.path != 0).any(axis=2)
    unstable = ranged & ~r.stable
    print("%s: %d pixels with candidates, %d unstable; general path: %d entries, max |f32 - f64| = %.3g"
          % (tag, ranged.sum(), unstable.sum(), gen.sum(), dg.max()))
    assert unstable.sum() <= 0.01 * ranged.sum(), "%s: %d of %d pixels unstable: a bad input" % (tag, unstable.sum(), ranged.sum())


def _f(x):
    return np.float32(x)


def test_a_nan_value_stores_the_clamp():
    """Hand-built windows (r = 2, every weight 1, integer values: every product and sum below is exact in double, so rounding
    the double expression to float once IS the fused operation).
      * A flat other-view window under two sweeps: every b_t is 0, s1 = s3 = 0, v = 0/0 -> the clamp.
      * The same under one pass: q3 = U - m (2P - T m) is the rounding residue of T (r - m)^2 = 0.  The value 821 (not a
        gray an image holds; the window call takes any double) makes U = 25 * 821^2 = 16 851 025 round to 16 851 024 on the
        last step of its chain while m (2P - T m) is exact: q3 = -1 (recomputed here), sqrtf of it is NaN -> the clamp.
      * A window with an unusable tap takes the general path."""
    import oracle_ffi as O
    op = O.params_twoview(window_radius=2)
    T = 25
    w = np.ones(T)
    l = np.arange(T, dtype=np.float64) * 3.0 + 7.0
    found = 821
    P, Uu = _f(0), _f(0)
    for t in range(T):
        P = _f(np.float64(found) + np.float64(P))
        Uu = _f(np.float64(found * found) + np.float64(Uu))
    m = _f(np.float64(P) * np.float64(_f(1.0) / _f(T)))
    i = _f(np.float64(P) + np.float64(P) - np.float64(T) * np.float64(m))
    q3 = _f(np.float64(Uu) - np.float64(m) * np.float64(i))
    assert q3 == -1.0, "the hand-built window no longer has a negative one-pass residue: %r" % q3
    r = np.full(T, float(found))
    path, f, B, lo = F.window(w, l, r, op)
    assert path == F.FAST
    assert f[0] == op.max_color_diff and f[1] == op.max_color_diff, (found, f)
    assert lo[0] == 1 and lo[1] == 1                      # s3 = 0: no first-order bound
    # a textured window stores its value below the clamp, the same in both forms to float accuracy
    r2 = l[::-1].copy()
    path, f, B, lo = F.window(w, l, r2, op)
    assert path == F.FAST and not lo.any() and np.all(f < op.max_color_diff) and np.all(np.isfinite(B))
    assert f[0] == np.float32(f[0]) and abs(f[0] - f[1]) <= 2 * (B[0] + B[1])
    r3 = r2.copy()
    r3[7] = np.nan
    path, f, B, lo = F.window(w, l, r3, op)
    assert path == F.GENERAL and f[0] == f[1] and np.isnan(B).all()
