"""GPU tests of shared_merge_kernel alone (csrc/aux.hip, through nvsr_shared_merge), the merge of the one-decoder render route: exact, against
the stable sort of tests/shared_merge_ref.py, on buffers the test owns.

  inputs ........ the coarse depths are nvsr_coarse_z's on the same packed rays (held bit for bit to what the kernels recompute by
                  test_depths_in_registers and the resampler tests); the sample lists are (a) nvsr_sample_pdf's on the mid-points for flat,
                  spiked and random weights, (b) samples equal to coarse depths, (c) all below / all above the coarse depths, (d) unsorted with
                  repeated values, (e) NaN in all samples / at the front, in the middle and at the end, (f) +inf samples, sorted and not, (g) a
                  NaN near; rays with near == far in every list and a list of nothing else
  outputs ....... z_merged and raw_merged hold a sentinel bit pattern before the launch and none after it; raw_coarse and raw_new carry exact
                  integer tags (ray, index, list): every slot holds the element whose depth stands in that slot, every element stands in exactly
                  one slot; both outputs equal the reference bit for bit.  One kind carries random bit patterns instead of tags (NaN payloads,
                  infinities) and is compared through the int32 view like all others: the 16-byte gather is a verbatim copy.
  shapes ........ N = 1, 5, 259 (four waves per workgroup: the last workgroup partial) by (Nc, Nf) = (3, 1), (4, 2), (63, 65), (64, 128),
                  (65, 129), (255, 256), (256, 256), (256, 1) (both ends of the LDS rows, both sides of a 64-lane stride), linear and lindisp

What these tests found (MI355X, profiles/shared_merge_edges.txt): ranked with plain < / <= / ==, the kernel sent every NaN element of a ray to
slot 0 and left as many slots of both outputs unwritten -- all 64 cases of the four NaN kinds failed, the lone NaN sample (Nf = 1) through
the binary searches.  The ranks now use rank_sort_wave's predicate.  242 tests in 1.6 s.
"""
import time

import numpy as np
import pytest
import torch

import shared_merge_ref as ref
from nerf_baseline_checks import DEV, T

pytestmark = pytest.mark.gpu

T0 = time.time()


def N_(t):
    return t.detach().cpu().numpy()


def _coarse_z(capi):
    def f(rays, Nc, lindisp):
        z, r_ = torch.full((rays.shape[0], Nc), float("nan"), device=DEV), T(rays)
        capi.call("nvsr_coarse_z", rays.shape[0], Nc, capi.ptr(r_), int(lindisp), None, capi.ptr(z), capi.stream())
        return N_(z)
    return f


def _sample_pdf(capi):
    def f(bins, w, ns):
        out, b_, w_ = torch.full((bins.shape[0], ns), float("nan"), device=DEV), T(bins), T(w)
        capi.call("nvsr_sample_pdf", bins.shape[0], bins.shape[1], ns, capi.ptr(b_), capi.ptr(w_), None, capi.ptr(out), capi.stream())
        return N_(out)
    return f


def merge(capi, c):
    """nvsr_shared_merge on a case -> z_merged [N,S], raw_merged [N,S,4] as int32 bit patterns; the outputs hold the sentinel before the launch"""
    S = c.Nc + c.Nf
    z_m = torch.full((c.N, S), ref.SENTINEL, dtype=torch.int32, device=DEV)
    raw_m = torch.full((c.N, S, 4), ref.SENTINEL, dtype=torch.int32, device=DEV)
    rays, b, raw_c, raw_new = T(c.rays), T(c.b), T(c.raw_c), T(c.raw_new)
    capi.call("nvsr_shared_merge", c.N, c.Nc, c.Nf, capi.ptr(rays), int(c.lindisp), capi.ptr(b), capi.ptr(raw_c), capi.ptr(raw_new), capi.ptr(z_m),
              capi.ptr(raw_m), capi.stream())
    torch.cuda.synchronize()
    return N_(z_m), N_(raw_m)


@pytest.mark.parametrize("p", ref.params(), ids=ref.case_id)
def test_merge_equals_the_stable_sort(hip, p):
    capi = hip.capi
    kind, (Nc, Nf), lindisp = p
    for N in ref.RAY_COUNTS:
        c = ref.build(kind, N, Nc, Nf, lindisp, _coarse_z(capi), _sample_pdf(capi))
        S, tag = Nc + Nf, "%s N=%d" % (ref.case_id(p), N)
        z_m, raw_m = merge(capi, c)
        order, z_ref, raw_ref = ref.merge_ref(c.a, c.b, c.raw_c, c.raw_new)
        left = (z_m == ref.SENTINEL).sum(-1) + (raw_m == ref.SENTINEL).any(-1).sum(-1)
        assert not left.any(), "%s: %d slots of z_merged / raw_merged unwritten (first on ray %d)" % (tag, int(left.sum()), int(np.flatnonzero(left)[0]))
        if kind != "bits":
            cat = np.concatenate([c.a, c.b], -1).view(np.int32)
            t = raw_m.view(np.float32).astype(np.int64)
            src = t[..., 2] * Nc + t[..., 1]
            assert np.array_equal(t[..., 0], np.broadcast_to(np.arange(N)[:, None], (N, S))), tag + ": an element of another ray"
            assert ((t[..., 2] == 0) | (t[..., 2] == 1)).all() and (src >= 0).all() and (src < S).all(), tag
            assert np.array_equal(t[..., 3], (2 * t[..., 0] + t[..., 2]) * 256 + t[..., 1]), tag + ": a 16-byte element torn"
            assert np.array_equal(np.take_along_axis(cat, src, -1), z_m), tag + ": a slot holds another element's decoder outputs than its depth's"
            assert np.array_equal(np.sort(src, -1), np.broadcast_to(np.arange(S), (N, S))), tag + ": an element stands in two slots or in none"
        bad = np.flatnonzero((z_m != z_ref).any(-1) | (raw_m != raw_ref).any((-1, -2)))
        assert bad.size == 0, "%s: %d rays differ from the reference, first ray %d:\nz %s\nref %s" % (
            tag, bad.size, bad[0], z_m[bad[0]].view(np.float32), z_ref[bad[0]].view(np.float32))


def test_no_rays_is_ok(hip):
    capi = hip.capi
    x = torch.zeros(16, device=DEV)
    capi.call("nvsr_shared_merge", 0, 64, 128, capi.ptr(x), 0, capi.ptr(x), capi.ptr(x), capi.ptr(x), capi.ptr(x), capi.ptr(x), capi.stream())
    torch.cuda.synchronize()
    assert not x.any()


def test_wall_time_of_this_file():
    print("shared_merge wall | %.1f s since the module was imported" % (time.time() - T0))
