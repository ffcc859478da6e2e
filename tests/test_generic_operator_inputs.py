"""Every operator of the generic decoder geometries on STRIDED inputs: ops._generic_call owns every .contiguous() of these operators, and a
dropped one fails silently -- the kernel reads the view's storage as a dense buffer.  Each operator is called once on contiguous tensors
and once on views of wider tensors that hold the same values (x, natural, packed, g_out / d_out as slices between junk columns or
elements, coord_noise as a transposed view); the outputs must be the same BITS.  No tolerance is involved.

Shapes: a hidden-32 'concat' / 'concat_pos' and a hidden-64 'sum' / 'mult' geometry on 8 x 8 planes; P = 1, 33 (one past a wave's 32 points)
and 129 (one past a four-wave workgroup's 128).

The two backward operators add with float atomics, whose order is not fixed.  Their cotangent is therefore nonzero on two rows only -- the
first and the last point, which are placed so that their 2 x 2 tap footprints share no texel on any plane (asserted below) -- and exactly
zero on every other row: a zero row contributes exact zeros, so every texel and every decoder weight receives at most the commutative sum of
two addends per decoder, and the result does not depend on the order.  The junk between the strided rows is nonzero, so a kernel that read
the cotangent's storage densely would not see those zeros."""
import numpy as np
import pytest
import torch

from test_generic_train_fused import seeded_model
from test_hip_parity import DEV, T

pytestmark = pytest.mark.gpu
GEOMETRIES = {
    "concat_concat_pos_32": dict(dec_channels=32, proj_combination="concat", viewdir_proj_combination="concat_pos"),
    "sum_mult_64": dict(dec_channels=64, proj_combination="sum", viewdir_proj_combination="mult"),
}
SIZE = 8
JUNK = 7.25
F32, F16X2 = 0, 2


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def strided(t):
    """the values of t as a view of a wider tensor: every second element of a vector, the middle columns of a matrix"""
    if t.dim() == 1:
        wide = torch.full((2 * t.numel() + 1,), JUNK, dtype=t.dtype, device=t.device)
        wide[::2][:t.numel()] = t
        v = wide[::2][:t.numel()]
    else:
        wide = torch.full((t.shape[0], t.shape[1] + 3), JUNK, dtype=t.dtype, device=t.device)
        wide[:, 1:1 + t.shape[1]] = t
        v = wide[:, 1:1 + t.shape[1]]
    assert torch.equal(bits(v), bits(t)) and (t.numel() <= 1 or t.shape[0] == 1 or not v.is_contiguous())
    return v


def transposed(t):
    v = t.t().contiguous().t()
    assert torch.equal(v, t) and (t.shape[0] == 1 or not v.is_contiguous())
    return v


def two_disjoint_points(consts):
    """two points whose bilinear footprints are disjoint on the three 8 x 8 position planes and on the 8 x 8 view plane (align_corners:
    texel = (g + 1) * 3.5), with room for the jitter of the test (1e-3 of the normalised range: 0.004 texels)"""
    lo, rng = np.array(consts[:5], np.float32), np.array(consts[5:10], np.float32)
    tex = np.array([[1.3, 1.45, 1.6], [4.3, 4.45, 4.6]], np.float32)
    vtex = np.array([[1.5, 1.4], [4.5, 4.4]], np.float32)
    xyz = lo[:3] + tex / np.float32(SIZE - 1) * rng[:3]
    az, el = lo[3] + vtex[:, 0] / (SIZE - 1) * rng[3], lo[4] + vtex[:, 1] / (SIZE - 1) * rng[4]
    x = np.concatenate([xyz, np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)], 1)], 1).astype(np.float32)
    n = (2 * (x[:, :3] - lo[:3]) / rng[:3] - 1).astype(np.float32)
    a2 = np.arctan2(x[:, 4], x[:, 3]).astype(np.float32)
    e2 = np.arctan2(x[:, 5], np.sqrt(x[:, 3] ** 2 + x[:, 4] ** 2)).astype(np.float32)
    grids = [n @ np.array(consts[10 + 6 * d:16 + 6 * d], np.float32).reshape(3, 2) for d in range(3)]
    grids.append(np.stack([2 * (a2 - lo[3]) / rng[3] - 1, 2 * (e2 - lo[4]) / rng[4] - 1], 1).astype(np.float32))
    for grid in grids:
        t = (grid + 1) * np.float32((SIZE - 1) / 2)
        fl = np.floor(t)
        assert np.all(fl >= 0) and np.all(fl + 1 <= SIZE - 1) and np.all(t - fl > 0.05) and np.all(t - fl < 0.95)
        cells = [{(int(fl[i, 1]) + dy, int(fl[i, 0]) + dx) for dy in (0, 1) for dx in (0, 1)} for i in range(2)]
        assert not (cells[0] & cells[1])
    return x


@pytest.fixture(scope="module", params=list(GEOMETRIES))
def scene(request, hip):
    """(planes, consts, geometry, natural, packed) of a seeded model of the geometry on 8 x 8 planes"""
    m, _ = seeded_model(hip, 11, size=SIZE, view_size=SIZE, **GEOMETRIES[request.param])
    planes, consts = m.scene_args(planes=[m.channel_last_plane(d).detach() for d in range(4)], check_native=False)
    natural, geometry = m.natural_blob().detach(), m.generic_geometry()
    return planes, consts, geometry, natural, torch.ops.nvsr.pack_generic_decoder(natural, geometry, 3)


def inputs(consts, natural, packed, P):
    rng = np.random.default_rng(100 + P)
    x = np.concatenate([rng.uniform(-4.3, 4.3, (P, 3)), rng.standard_normal((P, 3))], 1).astype(np.float32)
    ends = two_disjoint_points(consts)
    x[0], x[-1] = ends[0], ends[-1 if P > 1 else 0]
    g = np.zeros((P, 4), np.float32)
    g[0], g[-1] = rng.standard_normal(4), rng.standard_normal(4)
    w = rng.standard_normal(P).astype(np.float32)
    w[rng.random(P) < 0.4] = 0.0
    index = np.concatenate([rng.permutation(P), [0, 0]]).astype(np.int32)          # longer than max_count = P; the count is below it
    v = dict(x=T(x), natural=natural, packed=packed, noise=T((1e-3 * rng.standard_normal((P, 3))).astype(np.float32)), g=T(g), w=T(w),
             raw=T(rng.standard_normal((P, 4)).astype(np.float32)), index=T(index), count=T(np.array([2 * P // 3], np.int32)), max_count=P)
    views = dict(v, x=strided(v["x"]), natural=strided(natural), packed=strided(packed), noise=transposed(v["noise"]), g=strided(v["g"]),
                 w=strided(v["w"]), raw=strided(v["raw"]))
    return v, views


def run_all(planes, consts, geometry, v):
    """every generic operator on the tensors of v -> {name: output tensor}"""
    nv = torch.ops.nvsr
    tail = (True, v["noise"], False)
    head = (planes, consts, v["natural"])
    out = {"decode": nv.triplane_decode_generic(*head, geometry, v["x"], *tail),
           "fused": nv.triplane_decode_generic_fused(*head, geometry, v["x"], *tail),
           "pack": nv.pack_generic_decoder(v["natural"], geometry, 3)}
    grid = None
    for arith in (F32, F16X2):
        a = "/%d" % arith
        out["arith" + a] = nv.triplane_decode_generic_fused_arith(*head, v["packed"], geometry, v["x"], *tail, arith)
        out["density" + a] = nv.triplane_density_generic_fused_arith(*head, v["packed"], geometry, v["x"], *tail, arith)
        for name, op in (("colour", nv.triplane_colour_generic_fused_arith), ("density_list", nv.triplane_density_list_generic_fused_arith)):
            raw = torch.full((v["x"].shape[0], 4), JUNK, dtype=torch.float32, device=DEV)
            op(raw, *head, v["packed"], geometry, v["x"], v["index"], v["count"], *tail, arith, v["max_count"])
            out[name + a] = raw
        grid = nv.generic_occupancy_build(*head, v["packed"], geometry, 4, 1, 0.0, 1, True, False, arith)
        out["occupancy_build" + a] = grid
    index, count = nv.generic_live_list(v["w"])
    out["live_count"], out["live_index"] = count, index[:int(count.item())]          # (index[count:] is not written)
    out["keep"], out["keep_raw"] = nv.generic_occupancy_keep(consts, v["x"], grid, 4, v["raw"])
    for d, t in enumerate(nv.triplane_decode_generic_backward(*head, geometry, v["x"], v["g"], True, [True] * 4, *tail)):
        out["backward.%d" % d] = t
    for d, t in enumerate(nv.triplane_decode_generic_fused_backward(*head, geometry, v["x"], v["g"], [True] * 4, *tail)):
        out["fused_backward.%d" % d] = t
    return out


@pytest.mark.parametrize("P", [1, 33, 129])
def test_strided_inputs_give_the_bits_of_contiguous_ones(scene, P):
    planes, consts, geometry, natural, packed = scene
    dense, views = inputs(consts, natural, packed, P)
    with torch.no_grad():
        want, got = run_all(planes, consts, geometry, dense), run_all(planes, consts, geometry, views)
    torch.cuda.synchronize()
    assert list(want) == list(got)
    differ = [k for k in want if not same_bits(want[k], got[k])]
    assert not differ, differ
    # the operators did run: finite, nonzero outputs in f32, gradients on every plane and on the decoder
    for k in ("decode", "fused", "arith/0", "backward.0", "backward.1", "backward.4", "fused_backward.0", "fused_backward.3"):
        assert torch.isfinite(want[k]).all() and want[k].abs().max() > 0, k
    assert same_bits(want["fused"], want["decode"]) and same_bits(want["arith/0"], want["decode"])
    # the list operators: rows outside index[:count] keep what they held, and so does what a listed row's phase does not write
    listed = dense["index"][:int(dense["count"].item())].long()
    assert len(listed) < dense["max_count"] < len(dense["index"])
    rest = torch.ones(P, dtype=torch.bool, device=DEV)
    rest[listed] = False
    for arith in (F32, F16X2):
        for name in ("colour", "density_list"):
            raw = want["%s/%d" % (name, arith)]
            assert (raw[rest] == JUNK).all(), (name, arith)
        assert (want["colour/%d" % arith][:, 3] == JUNK).all()
        assert same_bits(want["colour/%d" % arith][listed][:, :3], want["arith/%d" % arith][listed][:, :3])
        assert same_bits(want["density_list/%d" % arith][listed][:, 3], want["density/%d" % arith][listed][:, 3])
