"""numpy statements of the generic geometries' frame in two phases (csrc/generic_live.hip, the phases of csrc/generic_fused*.hip): the live
list of a weight array, what the raw tensor holds after each phase in terms of the one-launch raw tensor, and the fc_alpha bias shift that
gives a wanted live share -- chosen from float64 sigmas alone."""
import numpy as np


def live_list(w):
    """the ascending flat positions p with not (w[p] == 0): NaN is live, +0.0 and -0.0 are dead"""
    return np.flatnonzero(~(np.asarray(w, np.float32).ravel() == 0)).astype(np.int32)


def density_raw(one_phase):
    """[P,4] after the density phase: [+0, +0, +0, sigma] with the one-launch tensor's sigma"""
    one_phase = np.asarray(one_phase, np.float32)
    out = np.zeros_like(one_phase)
    out[:, 3] = one_phase[:, 3]
    return out


def colour_raw(before, one_phase, index):
    """`before` [P,4] after a colour phase on the points `index`: their columns 0:3 are the one-launch tensor's, nothing else moves"""
    out = np.array(before, np.float32, copy=True)
    index = np.asarray(index, np.int64)
    out[index, :3] = np.asarray(one_phase, np.float32)[index, :3]
    return out


def two_phase_raw(one_phase, w):
    """the completed raw tensor of a two-phase pass whose weights are w"""
    return colour_raw(density_raw(one_phase), one_phase, live_list(w))


def bias_shift_for_share(sigma64, share):
    """s such that the fraction of sigma64 + s > 0 is `share` (as near as the sample allows): fc_alpha's bias enters sigma additively, and a
    sample whose sigma is not positive has alpha = 1 - exp(-relu(sigma) dist) = 0, hence weight 0"""
    s = np.sort(np.asarray(sigma64, np.float64).ravel())
    k = int(round((1.0 - share) * s.size))
    k = min(max(k, 1), s.size - 1)
    return -0.5 * (s[k - 1] + s[k])


def live_share(w):
    w = np.asarray(w)
    return live_list(w).size / float(w.size)
