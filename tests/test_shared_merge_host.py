"""CPU tests around shared_merge_kernel (csrc/aux.hip), on the case lists of the GPU test (tests/shared_merge_ref.py; the coarse depths and the
resampled lists come from numpy stand-ins here, the cases are of the same kinds and shapes):

  * the reference's values against torch.sort on the CPU, NaN rows included, and the reference against itself: the gathered decoder outputs
    name every element once, and each stands in the slot of its own depth;
  * a numpy transcription of the kernel's rank rules -- its choice between them, the two binary searches, the counting over [a | b] -- against
    the reference;
  * the counting rule as it was before the ranks became NaN-aware (plain < / <= / ==): equal to the reference on every ray without a NaN, and on
    every ray with one it sends two elements to one slot and leaves a slot unwritten -- the defect the GPU test's NaN cases exist for;
  * nvsr_shared_merge's argument checks (no launch: nothing here needs a GPU).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import shared_merge_ref as ref

PARAMS = ref.params()


def linspace01(n):
    """nvsr_common.h linspace01 in float32"""
    if n == 1:
        return np.zeros(1, np.float32)
    i = np.arange(n)
    step = np.float32(1) / np.float32(n - 1)
    return np.where(i < n // 2, step * i.astype(np.float32), np.float32(1) - step * (n - 1 - i).astype(np.float32)).astype(np.float32)


def coarse_z_np(rays, Nc, lindisp):
    """nvsr_common.h coarse_depth, operation by operation in float32"""
    t, nr, fr, one = linspace01(Nc)[None], rays[:, 6:7], rays[:, 7:8], np.float32(1)
    with np.errstate(invalid="ignore", divide="ignore"):
        z = nr * (one - t) + fr * t if not lindisp else one / ((one / nr) * (one - t) + (one / fr) * t)
    return np.ascontiguousarray(z, np.float32)


def sample_pdf_np(bins, w, ns):
    """inverse-CDF samples at u = linspace(0, 1, ns) (nerf_helpers.py:668-702) in float64: inputs of the right kind, not the kernel's bits"""
    N, nb = bins.shape
    u = linspace01(ns).astype(np.float64)
    w = w.astype(np.float64) + 1e-5
    cdf = np.concatenate([np.zeros((N, 1)), np.cumsum(w / w.sum(-1, keepdims=True), -1)], -1)
    out = np.empty((N, ns), np.float32)
    for r in range(N):
        idx = np.searchsorted(cdf[r], u, side="right")
        below, above = np.maximum(idx - 1, 0), np.minimum(idx, nb - 1)
        c0, den = cdf[r, below], cdf[r, above] - cdf[r, below]
        den = np.where(den < 1e-5, 1.0, den)
        out[r] = bins[r, below] + (u - c0) / den * (bins[r, above].astype(np.float64) - bins[r, below])
    return out


def _case(kind, shape, lindisp, N):
    return ref.build(kind, N, shape[0], shape[1], lindisp, coarse_z_np, sample_pdf_np)


def _search(arr, v, or_equal):
    """the kernel's binary search, one per element of v: lo = 0, hi = n; while (lo < hi) { mid; if (arr[mid] < v  [<= v]) lo = mid + 1; else hi = mid; }"""
    lo, hi = np.zeros(v.shape, np.int64), np.full(v.shape, arr.size, np.int64)
    while (lo < hi).any():
        act, mid = lo < hi, (lo + hi) >> 1
        x = arr[np.minimum(mid, arr.size - 1)]
        go = act & ((x <= v) if or_equal else (x < v))
        lo, hi = np.where(go, mid + 1, lo), np.where(act & ~go, mid, hi)
    return lo


def _counted(a, b, nan_aware):
    """positions by counting over all = [a | b]: #{k : all[k] stands before all[e]}"""
    v = np.concatenate([a, b])
    o, first = v[None, :], np.arange(v.size)[None, :] < np.arange(v.size)[:, None]
    lt, eq = o < v[:, None], o == v[:, None]
    if not nan_aware:                # a coarse depth: #(b < v) + #(a < v or a == v, earlier); a sample: #(a <= v) + #(b < v or b == v, earlier)
        return (lt | (eq & first)).sum(1)
    onan, vnan = np.isnan(o), np.isnan(v)[:, None]
    return (lt | (~onan & vnan) | ((eq | (onan & vnan)) & first)).sum(1)


def kernel_positions(a, b, nan_aware, force_counting=False):
    """the slot shared_merge_kernel writes each element of [a | b] to (clamped to the row, as the kernel clamps)"""
    Nc, Nf = a.size, b.size
    fast = bool((a[:-1] <= a[1:]).all() and (b[:-1] <= b[1:]).all())
    if nan_aware:
        fast = fast and not np.isnan(b).any()
    if fast and not force_counting:
        pos = np.concatenate([np.arange(Nc) + _search(b, a, False), np.arange(Nf) + _search(a, b, True)])
    else:
        pos = _counted(a, b, nan_aware)
    return np.minimum(pos, Nc + Nf - 1)


def _rows(N):
    return sorted(set(range(min(N, 5))) | set(range(max(N - 2, 0), N)))


@pytest.mark.parametrize("p", PARAMS, ids=ref.case_id)
def test_reference_values_equal_torch_sort(p):
    for N in ref.RAY_COUNTS:
        c = _case(*p, N)
        S = c.Nc + c.Nf
        order, z_m, raw_m = ref.merge_ref(c.a, c.b, c.raw_c, c.raw_new)
        assert np.array_equal(np.sort(order, -1), np.broadcast_to(np.arange(S), (N, S)))
        cat = np.concatenate([c.a, c.b], -1)
        got, want = z_m.view(np.float32), torch.sort(torch.from_numpy(cat), -1).values.numpy()
        assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.nan_to_num(got, nan=-1.0), np.nan_to_num(want, nan=-1.0)), (ref.case_id(p), N)
        nan = np.isnan(got)
        assert (nan[:, 1:] >= nan[:, :-1]).all()                        # NaNs last
        if c.kind != "bits":                                            # the tags: every element once, in the slot of its own depth
            tag = raw_m.view(np.float32).astype(np.int64)
            src = tag[..., 2] * c.Nc + tag[..., 1]
            assert np.array_equal(tag[..., 0], np.broadcast_to(np.arange(N)[:, None], (N, S)))
            assert np.array_equal(np.sort(src, -1), np.broadcast_to(np.arange(S), (N, S)))
            assert np.array_equal(np.take_along_axis(cat.view(np.int32), src, -1), z_m)
            assert np.array_equal(src, order)
        # the cases are what their names say
        has_nan = np.isnan(cat).any(-1)
        assert has_nan.any() == (c.kind in ref.NAN_KINDS), c.kind
        if c.kind in ("nan_all", "nan_some"):
            assert has_nan.all()
        if c.kind == "ties":
            assert all(np.isin(c.b[r], c.a[r]).all() for r in range(N))
        if c.kind == "below":
            assert (c.b.max(-1) < c.a.min(-1)).all()
        if c.kind == "above":
            assert (c.b.min(-1) > c.a.max(-1)).all()
        if c.kind.startswith("inf"):
            assert np.isposinf(c.b).any(-1).all()
        if c.kind == "zero_width":                                      # near (1 - t) + far t rounds: equal to a few ulps, in no particular order
            assert (np.abs(c.a - c.rays[:, 6:7]) <= 4 * np.spacing(c.rays[:, 6:7])).all()
    if p[0] == "unsorted" and p[1][1] > 2:
        assert (np.diff(c.b, axis=-1) < 0).any() and (np.diff(np.sort(c.b, -1), axis=-1) == 0).any()


@pytest.mark.parametrize("p", PARAMS, ids=ref.case_id)
def test_rank_rules_equal_reference(p):
    """the transcription against the reference on rays of every list (the rule knows no neighbours: the first five and the last two rays)"""
    lost = 0
    for N in ref.RAY_COUNTS:
        c = _case(*p, N)
        S = c.Nc + c.Nf
        order = ref.merge_ref(c.a, c.b, c.raw_c, c.raw_new)[0]
        for r in _rows(N):
            a, b = c.a[r], c.b[r]
            want = np.argsort(order[r])                                  # the slot of element e of [a | b]
            tag = "%s N=%d ray %d" % (ref.case_id(p), N, r)
            assert np.array_equal(kernel_positions(a, b, True), want), tag
            assert np.array_equal(kernel_positions(a, b, True, force_counting=True), want), tag + " (counting)"
            old = kernel_positions(a, b, False)
            if np.isnan(a).any() or np.isnan(b).any():                  # the defect: NaN elements share slot 0, as many slots stay unwritten
                unwritten = S - np.unique(old).size
                assert unwritten > 0 and (old == 0).sum() > 1, tag
                lost += unwritten
            else:
                assert np.array_equal(old, want), tag + " (plain counting)"
                assert np.array_equal(kernel_positions(a, b, False, force_counting=True), want), tag + " (plain counting, forced)"
    assert (lost > 0) == (p[0] in ref.NAN_KINDS)


def test_plain_counting_on_the_example_of_the_defect():
    """Nc = 8, Nf = 12, every sample NaN (what a NaN or inf weight inside w[1:-1] makes of them): 12 slots unwritten, one slot written 13 times"""
    a, b = coarse_z_np(ref.make_rays("nan_all", 1, np.random.default_rng(0)), 8, 0)[0], np.full(12, np.nan, np.float32)
    old = kernel_positions(a, b, False)
    assert 20 - np.unique(old).size == 12 and (old == 0).sum() == 13
    assert np.array_equal(kernel_positions(a, b, True), np.arange(20))


def test_entry_point_checks_its_arguments():
    """NULL pointers, the alignment of the three raw pointers, the ranges of N, Nc and Nf; N == 0 is OK.  Every call returns before a launch."""
    import nvsr_amd
    nvsr_amd.build_extension()
    lib = nvsr_amd.capi.lib()
    OK, SHAPE, NULL, ALIGN = 0, 1, 3, 4
    buf = (C.c_float * 64)()
    base = (C.addressof(buf) + 15) & ~15
    good = dict(rays=base, z_new=base + 4, raw_c=base + 16, raw_new=base + 32, z_m=base + 8, raw_m=base + 48)

    def call(N=0, Nc=64, Nf=128, **kw):
        q = {k: C.c_void_p(v) if v else None for k, v in {**good, **kw}.items()}
        return lib.nvsr_shared_merge(N, Nc, Nf, q["rays"], 0, q["z_new"], q["raw_c"], q["raw_new"], q["z_m"], q["raw_m"], None)

    assert call() == OK
    for name in good:
        assert call(**{name: 0}) == NULL, name
    for name in ("raw_c", "raw_new", "raw_m"):
        for off in (4, 8, 12):
            assert call(**{name: good[name] + off}) == ALIGN, (name, off)
    assert call(z_new=base + 4, z_m=base + 12) == OK                    # the depth lists are read and written float by float
    assert call(N=-1) == SHAPE
    for Nc, Nf in ((2, 1), (257, 1), (3, 0), (3, 257), (0, 0), (-1, 5)):
        assert call(Nc=Nc, Nf=Nf) == SHAPE, (Nc, Nf)
    for Nc, Nf in ((3, 1), (256, 256)):
        assert call(Nc=Nc, Nf=Nf) == OK, (Nc, Nf)
