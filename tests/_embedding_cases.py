"""The cases of the morphology-embedding tests (tests/test_embedding_cpu.py, tests/test_gpu_embedding.py) and the constants measured on
them -- on the CPU, never from the device's output."""
import functools

import numpy as np

from syconn_amd.cnn.viewnet_spec import TNET_REP, ViewNetSpec

import _embedding_ref as E
import _viewnet_ref as R
from _viewnet_cases import C, C_REF, STORES, crc      # noqa: F401

Z = 25
# name -> (spec, H, W, n views).  g372: the window of the config; min: the smallest view the stack takes (92 -> 88 -> 44 -> 40 -> 20 -> 17
# -> 14 -> 7 -> 6 -> 3 -> 2 -> 1), 9 samples = one full tile of 8 and a tile of one; g6076: the module as written, 512 x 512.
GEOMS = {
    'g372': (TNET_REP(Z, 372), 128, 256, 5),
    'min': (TNET_REP(Z, 31), 92, 92, 9),
    'g6076': (TNET_REP(Z, 6076), 512, 512, 2),
}


@functools.lru_cache(maxsize=None)
def inputs(name: str):
    """(spec, H, W, arrs (convolution weights 5-D, exact in both storage types), views uint8 (n, 4, 2, H, W)) of a geometry, seeded."""
    spec, H, W, n = GEOMS[name]
    seed = 310 + sum(map(ord, name))
    return spec, H, W, E.make_weights(spec, seed, H, W), R.synthetic_views(seed + 7, n, 4, 2, H, W)


# The head A/B cases: the tiled head against the per-sample head, bit for bit.  12 x 12 views, two layers: 12 -> 8 -> 4 (k = 5, pool) ->
# 3 (k = 2); the tile size TS follows from the widest Linear alone: 4 TS (nin + 2 hmax) <= 160 KiB.
#   t8   9 x 6 + 0 = 54 -> 20 -> 7: TS = 8, D = 1, no scalar: the embedding's shape
#   t8s  D = 3, two scalars, LeakyReLU, two hidden Linear layers: TS = 8
#   t4   hidden 2600: 4 x 8 x (54 + 5200) > 160 KiB >= 4 x 4 x (54 + 5200): TS = 4
#   t1   12 -> 8 (k = 5) -> 8 (k = 1), 65 x 64 = 4160 features, hidden 8 then 8192 (the widest output alone sets the hidden tiles, so the
#        weights stay small: 4160 x 8 + 8 x 8192 + 8192 x 3): 4 x 2 x (4160 + 16384) > 160 KiB: TS = 1
HEAD_CASES = {
    't8': (ViewNetSpec(4, ((8, 5, 2), (6, 2, 1)), 54, (20,), 7, 0, 'relu', name='t8'), 1, 8),
    't8s': (ViewNetSpec(4, ((8, 5, 2), (6, 2, 1)), 162, (20, 11), 7, 2, 'leaky_relu', name='t8s'), 3, 8),
    't4': (ViewNetSpec(4, ((8, 5, 2), (6, 2, 1)), 54, (2600,), 7, 0, 'relu', name='t4'), 1, 4),
    't1': (ViewNetSpec(4, ((8, 5, 1), (65, 1, 1)), 4160, (8, 8192), 3, 0, 'relu', name='t1'), 1, 1),
}
HEAD_HW = 12
LDS_BYTES = 160 * 1024


def tile_samples(spec) -> int:
    """The rule of include/syconn_dense.h, restated: the largest of 8, 4, 2, 1 whose tiles fit 160 KiB."""
    sizes = spec.linear_sizes
    for ts in (8, 4, 2):
        if 4 * ts * (sizes[0] + 2 * max(sizes[1:])) <= LDS_BYTES:
            return ts
    return 1


def head_counts(ts: int, grid: int):
    """The sample counts of the A/B test: 1, TS - 1, TS, TS + 1, 3 TS + 5 and one more than a full grid stride of tiles."""
    return sorted({1, max(ts - 1, 1), ts, ts + 1, 3 * ts + 5, ts * grid + 1})


@functools.lru_cache(maxsize=None)
def head_inputs(name: str):
    """(spec, D, arrs, pool of 37 distinct locations uint8 (37, 4, D, 12, 12), scalars (37, n_scalar)); the samples of a count are
    drawn from the pool through the sample table.  The wide Linear layers are plain seeded normals (no probe pass: the A/B test
    compares bits, not magnitudes)."""
    spec, D, _ = HEAD_CASES[name]
    seed = 500 + sum(map(ord, name))
    rng = np.random.default_rng(seed)
    shapes = list(spec.param_shapes().values())
    nl = len(spec.layers)
    arrs = []
    for s in shapes:      # weights of unit gain per layer, small biases: no layer dies behind its activation
        a = rng.standard_normal(s, dtype=np.float32)
        arrs.append(a * np.float32(2.0 / np.sqrt(np.prod(s[1:]))) if len(s) > 1 else a * np.float32(0.1))
    views = R.synthetic_views(seed + 7, 37, 4, D, HEAD_HW, HEAD_HW)
    return spec, D, arrs, views, rng.uniform(-1, 1, (37, spec.n_scalar)).astype(np.float32)


# -- measured on the CPU ------------------------------------------------------------------------------------------------------------------
# The accumulation constant of the layer shapes of this net (k = 4 without a pool, k = 2 with a pool twice, 13 ... 31 channels), measured
# by tests/test_embedding_cpu.py::test_accumulation_constant as in tests/_viewnet_cases.py: the largest |ref32 - ref64| / (2^-24 S) of any
# op of g372, min and g6076 on the inputs the float64 chain produces.  It stays below C_REF of _viewnet_cases.py (4.873 / 2.632), so the
# bound of tests/test_gpu_viewnet.py, c = 4 C_REF, is used unchanged.
C_REF_MEASURED = {'f16': 3.712, 'bf16': 2.591}      # both set by g372's layers; 1 and 16 threads gave the same maxima

# T = 4 x the largest |emulation - float32 restatement| of the latents of a case, both on the stored weights (E.latent_emul,
# E.latent32): activation rounding only.  Measured by tests/test_embedding_cpu.py::test_tolerance, which recomputes it; the golden
# cases (tests/golden/make_golden_embedding.py) are measured on their own generated inputs.
# (1 thread / 16 threads differ in the fourth digit at most; recorded: the smaller.)  The latents are of order 1 (largest 3.3 to 4.7).
EMUL_DIFF = {
    'g372': {'f16': 0.0024232864, 'bf16': 0.016727567},
    'min': {'f16': 0.0023291595, 'bf16': 0.018109322},
    'g6076': {'f16': 0.0021032691, 'bf16': 0.017127037},
    'golden_lit': {'f16': 0.0043942928, 'bf16': 0.021009207},
    'golden_w372': {'f16': 0.0014992729, 'bf16': 0.013384819},
}
T = {case: {s: 4.0 * v for s, v in d.items()} for case, d in EMUL_DIFF.items()}


# -- the golden of the reference's own functions (tests/golden/make_golden_embedding.py -> g31_embedding.npz) ----------------------------
GOLDEN_SEED = 3100
GOLDEN = {'lit': ('g6076', 2, 2), 'w372': ('g372', 6, 2)}      # name -> (geometry, locations, views per location)
GOLDEN_SCALING = np.array([10., 10., 20.], np.float32)


@functools.lru_cache(maxsize=None)
def golden_weights(name: str):
    geom = GOLDEN[name][0]
    spec, H, W, _ = GEOMS[geom]
    return E.make_weights(spec, GOLDEN_SEED + sum(map(ord, name)), H, W)


@functools.lru_cache(maxsize=None)
def golden_cell(name: str):
    """(views uint8 (n_loc, 4, vpl, H, W), locations float32 (n_loc, 3) nm, nodes int64 (m, 3) voxels) of a golden cell.  Locations sit
    on a coarse lattice; the nodes are seeded draws plus, for w372, five constructed ties -- nodes exactly half way between two
    locations (both float64 distances are the same number: sums of squares of small integers; the rows of the two are whatever the
    seeded permutation of the lattice gave them) -- and one node that sits on a location.  One of the 30 seeded draws happens to be
    equidistant from two locations as well, so the stored golden counts six ties."""
    geom, n_loc, vpl = GOLDEN[name]
    spec, H, W, _ = GEOMS[geom]
    seed = GOLDEN_SEED + 17 * sum(map(ord, name))
    rng = np.random.default_rng(seed)
    views = R.synthetic_views(seed, n_loc, 4, vpl, H, W)
    lattice = np.array([[0, 0, 0], [400, 0, 0], [0, 600, 0], [400, 600, 200], [800, 0, 400], [800, 600, 400]], np.float32)
    order = rng.permutation(len(lattice))[:n_loc]
    locs = lattice[order]
    n_rand = 30 if name == 'w372' else 5
    nodes = np.stack([rng.integers(-10, 95, n_rand), rng.integers(-10, 75, n_rand), rng.integers(-5, 25, n_rand)], 1).astype(np.int64)
    if name == 'w372':
        sc = GOLDEN_SCALING.astype(np.float64)
        # lattice neighbours: no third location is as near to their midpoint, whatever rows the permutation gave them
        mids = [(lattice[a].astype(np.float64) + lattice[b]) / 2 for a, b in ((0, 1), (2, 3), (4, 5), (1, 4), (3, 5))]
        extra = np.array([m / sc for m in mids] + [locs[3].astype(np.float64) / sc])
        assert np.array_equal(extra, np.rint(extra))
        nodes = np.concatenate([nodes[:11], extra[:3].astype(np.int64), nodes[11:], extra[3:].astype(np.int64)])
    return views, locs, nodes
