"""numpy restatement of nvsr_rows_scatter's contract (include/nvsr.h), shared by tests/test_deterministic_host.py (checked against a
float64 sum) and tests/test_deterministic.py (the GPU result must equal it bit for bit)."""
import numpy as np


def rows_scatter_ref(rows, texel, weight, g):
    """rows [M,48] f32, texel [M,4] int32, weight [M,4] f32, g [H,W,48] f32 -> a copy of g with the rows added, in float32 throughout:
    entry e = 4 m + j belongs to texel texel[e]; per texel named by an entry and per channel, s starts from +0.0 and adds
    fl(rows[m][c] * weight[e]) over the texel's entries in ascending e; then g[t][c] = fl(g[t][c] + s).  Every entry takes part."""
    assert rows.dtype == weight.dtype == g.dtype == np.float32 and texel.dtype == np.int32
    out = g.copy()
    flat = out.reshape(-1, g.shape[-1])
    tex, w = texel.reshape(-1), weight.reshape(-1)
    order = np.argsort(tex, kind="stable")                  # ascending e inside a texel
    bounds = np.flatnonzero(np.diff(tex[order])) + 1
    with np.errstate(invalid="ignore", over="ignore"):
        for seg in np.split(order, bounds):
            if seg.size == 0:
                continue
            s = np.zeros(g.shape[-1], np.float32)
            for e in seg:
                s = s + rows[e >> 2] * w[e]                 # float32 product rounded, then float32 sum rounded
            t = tex[seg[0]]
            flat[t] = flat[t] + s
    return out


def rows_scatter_f64(rows, texel, weight, g):
    """the same sums in float64 (np.add.at: any order) -> (result, sum of |terms| per element, entries per texel)"""
    C = g.shape[-1]
    out = g.astype(np.float64).reshape(-1, C).copy()
    mag = np.abs(out).copy()
    tex = texel.reshape(-1)
    terms = np.repeat(rows.astype(np.float64), 4, axis=0) * weight.reshape(-1, 1).astype(np.float64)
    np.add.at(out, tex, terms)
    np.add.at(mag, tex, np.abs(terms))
    count = np.bincount(tex, minlength=out.shape[0])
    return out.reshape(g.shape), mag.reshape(g.shape), count.reshape(g.shape[:-1])


def scatter_case(M, H, W, seed, kind="random"):
    """inputs of one rows_scatter case: g pre-filled with random NON-ZERO values (an untouched texel must keep its bits)"""
    rng = np.random.default_rng(seed)
    rows = rng.standard_normal((M, 48)).astype(np.float32)
    texel = rng.integers(0, H * W, (M, 4)).astype(np.int32)
    weight = rng.random((M, 4)).astype(np.float32)
    g = (rng.standard_normal((H, W, 48)) + 3.0).astype(np.float32)
    if kind == "one_texel":             # every entry on texel 0: one segment of 4 M entries
        texel[:] = 0
    elif kind == "zero_weights":        # weight 0 takes part like any other (a clamped neighbour): +0.0 / -0.0 products
        weight[rng.random((M, 4)) < 0.5] = 0.0
    elif kind == "nan_row":             # reaches exactly its four texels, zero weights included
        rows[M // 2] = np.nan
        weight[M // 2, 1] = 0.0
    else:
        assert kind == "random"
    return rows, texel, weight, g
