"""CPU checks of the g25 fixture (tests/golden/gen_golden_nerf_ragged.py): both FlexibleNeRFModel baselines at 7 x 11 rays and 33 + 17 samples,
whose passes are no multiple of the engine's 32-point tile (tests/test_nerf_baseline_edges.py runs them on the GPU)."""
import sys

import numpy as np
import pytest

from conftest import GOLDEN, load_golden

if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
import mip_params  # noqa: E402
import pe_params  # noqa: E402

OUTS = ("rgb_coarse", "disp_coarse", "acc_coarse", "rgb_fine", "disp_fine", "acc_fine")


@pytest.mark.parametrize("model", ["mip", "pe"])
def test_g25_fixture_keys_shapes_and_ragged_passes(model):
    g = {k[len(model) + 1:]: v for k, v in load_golden("g25_nerf_ragged.npz").items() if k.startswith(model + ".")}
    params, extra, div = (mip_params, 1, 4) if model == "mip" else (pe_params, 0, 1)
    H, W, _ = g["c.hwf"]
    n, nc, nf = int(H) * int(W), int(g["num_coarse"]), int(g["num_fine"])
    assert (n, nc, nf) == (77, 33, 17)
    for i, seed in enumerate(params.SEEDS):
        np.testing.assert_allclose(params.checksum(params.state_dict(seed)), g["b.m%d.checksum" % i], rtol=1e-12)
        for name, shape in params.SHAPES:
            assert g["d.m%d.grad.%s" % (i, name)].shape == (min(int(np.prod(shape)), params.KEEP),)
    assert g["c.ro"].shape == g["c.rd"].shape == (int(H), int(W), 3)
    for tag in ("c.", "c.ndc.", "d."):
        for key in OUTS:
            assert g[tag + key].shape == ((n, 3) if key.startswith("rgb") else (n,)), tag + key
    # the depths each pass ran at (Mip: interval edges, one more than the intervals): no pass is a whole number of tiles
    for tag in ("c.", "c.ndc."):
        zc, zf = g[tag + "z_coarse"], g[tag + "z_fine"]
        assert zc.shape == (n, nc + extra) and zf.shape == (n, nc + nf + 2 * extra)
        passes = [n * (zc.shape[1] - extra), n * (zf.shape[1] - extra)]
        assert passes == ([2541, 3927] if model == "mip" else [2541, 3850])
        assert all(P % 32 for P in passes), passes
        assert (np.diff(zc, axis=-1) >= 0).all() and (np.diff(zf, axis=-1) >= 0).all()
    assert g["d.target"].shape == (n, 3) and g["d.loss"].shape == ()
    # the reference draws the train step's random numbers per chunksize // div rays: at least two chunks, the last one partial
    rays = int(g["chunksize"]) // div
    assert n // rays >= 2 and n % rays, rays
