"""The definition that shared_merge_kernel (csrc/aux.hip, nvsr_shared_merge) is held to, in plain numpy, and the case lists of its tests
(tests/test_shared_merge.py on the GPU, tests/test_shared_merge_host.py on the CPU).

The kernel merges a ray's Nc coarse depths a (recomputed from the packed ray's near / far) with its Nf new samples b and gathers the two
lists of decoder outputs into the merged order.  Its rule -- a coarse depth goes behind the samples that are smaller, a sample behind the coarse
depths that are smaller or equal, ties inside a list go by index, NaNs go last (coarse before samples, by index), as torch.sort and
rank_sort_wave order them -- is one stable sort of [a | b]:

    order = argsort(cat(a, b), kind="stable");  z_m = cat(a, b)[order];  raw_m = cat(raw_c, raw_new)[order]

A permutation and a copy: the comparison is exact, bit patterns included (the gathers run on int32 views, so a NaN's payload survives).
"""
from types import SimpleNamespace as NS

import numpy as np

RAY_COUNTS = (1, 5, 259)           # one wave per ray, four waves per workgroup: every count leaves the last workgroup partial
# both ends of the kernel's LDS rows (256 floats each) and both sides of a 64-lane stride
SHAPES = ((3, 1), (4, 2), (63, 65), (64, 128), (65, 129), (255, 256), (256, 256), (256, 1))
KINDS = ("pdf_flat", "pdf_spiked", "pdf_random",                  # (a) the resampler's own samples
         "ties",                                                  # (b) every sample equal to a coarse depth
         "below", "above",                                        # (c) all samples outside the coarse depths
         "unsorted",                                              # (d) unsorted samples with repeated values
         "nan_all", "nan_some",                                   # (e) NaN samples: all; at the front, in the middle and at the end
         "inf_tail", "inf_mixed",                                 # (f) +inf samples: a sorted tail; out of order
         "nan_near", "nan_near_nan_samples",                      # (g) a NaN near: every coarse depth of the ray NaN
         "zero_width",                                            # near == far on every ray: all coarse depths equal to an ulp or two, often unsorted
         "bits")                                                  # decoder outputs of random bit patterns, NaN payloads included
NAN_KINDS = ("nan_all", "nan_some", "nan_near", "nan_near_nan_samples")
SENTINEL = 0x7FC0DEAD              # the bit pattern the outputs hold before the launch (a NaN with a payload no input carries)


def merge_ref(a, b, raw_c, raw_new):
    """a [N,Nc], b [N,Nf] float32, raw_c [N,Nc,4], raw_new [N,Nf,4] (float32 or int32 bit patterns) -> order [N,Nc+Nf], z_m, raw_m (int32 views)"""
    cat = np.concatenate([a, b], -1).astype(np.float32, copy=False)
    order = np.argsort(cat, -1, kind="stable")
    z_m = np.take_along_axis(np.ascontiguousarray(cat).view(np.int32), order, -1)
    raw = np.concatenate([np.ascontiguousarray(raw_c).view(np.int32), np.ascontiguousarray(raw_new).view(np.int32)], 1)
    raw_m = np.take_along_axis(raw, order[..., None], 1)
    return order, z_m, raw_m


def tags(N, Nc, Nf):
    """decoder outputs that name their element: (ray, index, list, id), exact integers in float32; id = (2 ray + list) 256 + index"""
    def one(n, lst):
        r, i = np.meshgrid(np.arange(N), np.arange(n), indexing="ij")
        return np.stack([r, i, np.full_like(r, lst), (2 * r + lst) * 256 + i], -1).astype(np.float32)
    return one(Nc, 0), one(Nf, 1)


def make_rays(kind, N, rng):
    """packed rays [N,11]: the kernel reads near and far (columns 6, 7); every fourth ray has near == far"""
    rays = np.zeros((N, 11), np.float32)
    near = rng.uniform(0.5, 2.5, N).astype(np.float32)
    far = near + rng.uniform(0.5, 5.0, N).astype(np.float32)
    far[1::4] = near[1::4]
    if kind == "zero_width":
        far = near.copy()
    if kind.startswith("nan_near"):
        near[0::2] = np.nan
    rays[:, 6], rays[:, 7] = near, far
    return rays


def _nan_some(b, value=np.nan):
    b = b.copy()
    Nf = b.shape[1]
    b[:, [0, Nf // 2, Nf - 1]] = value
    b[1::2, min(1, Nf - 1)] = value
    return b


def build(kind, N, Nc, Nf, lindisp, coarse_z, sample_pdf):
    """one case: NS(rays, a, b, raw_c, raw_new).  coarse_z(rays, Nc, lindisp) -> [N,Nc] and sample_pdf(bins [N,nb], w [N,nb-1], ns) -> [N,ns] are
    the caller's: the GPU test passes the library's kernels, the CPU test numpy stand-ins (the inputs need not be the same numbers, only of
    the same kind)."""
    rng = np.random.default_rng([KINDS.index(kind), N, Nc, Nf, lindisp])
    rays = make_rays(kind, N, rng)
    a = coarse_z(rays, Nc, lindisp)
    assert a.shape == (N, Nc) and a.dtype == np.float32

    def resampled(w):
        mid = (np.float32(0.5) * (a[:, 1:] + a[:, :-1])).astype(np.float32)
        return sample_pdf(mid, w.astype(np.float32), Nf)

    w_random = lambda: rng.uniform(0, 1, (N, Nc - 2)) ** 6
    uniform_sorted = lambda: np.sort(rng.uniform(2.0, 6.0, (N, Nf)).astype(np.float32), -1)
    if kind == "pdf_flat":
        b = resampled(np.zeros((N, Nc - 2)))
    elif kind == "pdf_spiked":
        w = np.zeros((N, Nc - 2))
        w[np.arange(N), rng.integers(0, Nc - 2, N)] = 50.0
        b = resampled(w)
    elif kind in ("pdf_random", "zero_width", "bits"):
        b = resampled(w_random())
    elif kind == "ties":
        b = np.take_along_axis(a, np.sort(rng.integers(0, Nc, (N, Nf)), -1), -1)
    elif kind == "below":
        b = a[:, :1] - np.float32(0.01) * (Nf - np.arange(Nf, dtype=np.float32))[None]
    elif kind == "above":
        b = a[:, -1:] + np.float32(0.01) * (1 + np.arange(Nf, dtype=np.float32))[None]
    elif kind == "unsorted":
        pool = np.concatenate([rng.uniform(rays[:, 6:7] - 0.5, rays[:, 7:8] + 0.5, (N, max(1, Nf // 3))).astype(np.float32), a[:, [0, Nc // 2, Nc - 1]]], -1)
        b = np.take_along_axis(pool, rng.integers(0, pool.shape[1], (N, Nf)), -1)
    elif kind == "nan_all":
        b = np.full((N, Nf), np.nan, np.float32)
    elif kind == "nan_some":
        b = _nan_some(resampled(w_random()))
    elif kind == "inf_tail":
        b = resampled(w_random())
        b[:, Nf - max(1, Nf // 4):] = np.inf
    elif kind == "inf_mixed":
        b = _nan_some(resampled(w_random()), np.inf)
    elif kind == "nan_near":
        b = uniform_sorted()
    elif kind == "nan_near_nan_samples":
        b = _nan_some(uniform_sorted())
    else:
        raise KeyError(kind)
    b = np.ascontiguousarray(b, np.float32)
    assert b.shape == (N, Nf)
    if kind == "bits":
        raw_c = rng.integers(-2 ** 31, 2 ** 31, (N, Nc, 4), dtype=np.int64).astype(np.int32)
        raw_new = rng.integers(-2 ** 31, 2 ** 31, (N, Nf, 4), dtype=np.int64).astype(np.int32)
        raw_c[0, 0], raw_new[0, 0] = [0x7FC00001, -0x3FFFFF, 0x7F800001, -0x800000], [0x7FFFFFFF, -1, 0x7FA00000, 0x7F800000]   # NaNs with payloads, quiet and signalling; -inf, +inf
        assert not (raw_c == SENTINEL).any() and not (raw_new == SENTINEL).any()
    else:
        raw_c, raw_new = tags(N, Nc, Nf)
    return NS(kind=kind, N=N, Nc=Nc, Nf=Nf, lindisp=lindisp, rays=rays, a=a, b=b, raw_c=raw_c, raw_new=raw_new)


def case_id(p):
    kind, (Nc, Nf), lindisp = p
    return "%s-%dx%d-%s" % (kind, Nc, Nf, "lindisp" if lindisp else "linear")


def params():
    return [(k, s, l) for k in KINDS for s in SHAPES for l in (0, 1)]
