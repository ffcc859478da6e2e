"""GPU test of the SR stage's one forward walk (csrc/sr.hip: edsr_forward_walk; DESIGN.md 3.3, "Host side of the SR route"): the inference
forward (three rotating buffers; nvsr_planes_sr_arith, nvsr_planes_sr_batch_arith with B = 1 and 3) and the training forward (the activation
record; nvsr_planes_sr_train_arith) launch the same kernels on the same grids, so their planes are the same bits -- per arithmetic, on the
narrow limb / exact-f32 narrow kernels (hidden 16) and the 16x16x32 kernels (hidden 128), on three regions of interest.  The same relation held
before the walks were folded into one (measured on the parent commit with this file: all 24 cases equal)."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
R = 24
ROIS = [[-0.9, -0.35, 0.1, 0.8], [-1.0, -1.0, 0.2, 0.3], [-0.2, -0.6, 0.95, 0.4]]      # (the second touches two borders: replicate padding)


@pytest.fixture(scope="module")
def hip():
    import nvsr_amd

    nvsr_amd.build_extension()
    return nvsr_amd


@pytest.fixture(scope="module")
def nets(hip):
    """(hid, n_blocks) -> (PlanesSR, three LR planes [48][R][R]), weights x 10 so that every layer's output has weight"""
    made = {}
    for hid, nb in ((16, 2), (128, 1)):
        torch.manual_seed(31)
        sr = hip.models.PlanesSR(hip.models.EDSR, 4, 48, 48, {"model": {"hidden_size": hid, "n_blocks": nb}}, "bilinear").to(DEV)
        with torch.no_grad():
            for p_ in sr.parameters():
                p_.mul_(10.0)
        g = torch.Generator(device=DEV).manual_seed(32)
        made[hid, nb] = (sr, [torch.randn(48, R, R, device=DEV, generator=g) * 0.5 for _ in range(3)])
    return made


def same_plane(a, b):
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))


@pytest.mark.parametrize("hid,nb", [(16, 2), (128, 1)])
@pytest.mark.parametrize("mode", ["f32", "bf16x3", "f16x2", "f16"])
def test_inference_and_training_forwards_give_the_same_planes(hip, nets, hid, nb, mode):
    capi = hip.capi
    lib = capi.lib()
    sr, lrs = nets[hid, nb]
    net = sr.inner_model
    cin, cout, hid_, nb_, n_up = net.geometry
    pad, over, sf = sr._kernel_pad, sr._kernel_over, 1 << n_up
    arith = capi.CONV_ARITHMETIC[mode]
    packed = net.packed_weights()
    new = lambda: torch.full((48, R * sf, R * sf), 7.0, device=DEV)
    for roi in ROIS:
        roi_c = (C.c_float * 4)(*roi)
        nws = lib.nvsr_planes_sr_workspace_floats(48, R, R, hid_, nb_, n_up, pad, roi_c)
        nkeep = lib.nvsr_planes_sr_keep_floats(48, R, R, hid_, nb_, n_up, pad, roi_c)
        assert nws > 0 and nkeep > 0
        ws = torch.empty(3 * nws, device=DEV)
        head = (48, R, R, capi.ptr(packed), hid_, nb_, n_up, pad, over, roi_c, None, None)
        one = new()
        capi.call("nvsr_planes_sr_arith", capi.ptr(lrs[0]), *head, capi.ptr(one), capi.ptr(ws), arith, capi.stream())
        assert bool(torch.isnan(one).any()) and bool(torch.isfinite(one).any()) and not bool((one == 7.0).any())
        batch = {}
        for B in (1, 3):
            outs = [new() for _ in range(B)]
            capi.call("nvsr_planes_sr_batch_arith", (C.c_void_p * B)(*[t.data_ptr() for t in lrs[:B]]), B, *head,
                      (C.c_void_p * B)(*[t.data_ptr() for t in outs]), capi.ptr(ws), arith, capi.stream())
            batch[B] = outs
        trained = []
        for k in range(3):
            out, keep = new(), torch.empty(nkeep, device=DEV)
            capi.call("nvsr_planes_sr_train_arith", capi.ptr(lrs[k]), *head, capi.ptr(out), capi.ptr(ws), capi.ptr(keep), arith, capi.stream())
            trained.append(out)
        assert same_plane(one, batch[1][0]) and same_plane(one, batch[3][0]) and same_plane(one, trained[0])
        assert all(same_plane(batch[3][k], trained[k]) for k in range(3))
        assert not same_plane(trained[0], trained[1])
