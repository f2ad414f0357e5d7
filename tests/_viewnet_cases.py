"""The cases of the view-net tests (tests/test_viewnet_cpu.py, tests/test_gpu_viewnet.py) and the constants measured on them."""
import functools
import zlib

import numpy as np

from syconn_amd.cnn.viewnet_spec import CELLTYPE_CMN, ViewNetSpec

import _viewnet_ref as R

STORES = ('f16', 'bf16')

# name -> (spec, D, H, W, n_samples).  What each one is there for:
#   a  23 x 37, k = 5, p = 2: conv 19 x 33 -> pool 9 x 16 drops one odd row and one odd column; 4 -> 20 -> 30 (K = 100, 500: no multiple
#      of 32); two tiles in x; D = 3; two scalars
#   b  12 x 9, k = 4; one input channel; LeakyReLU; D = 1; one scalar; a k = 1, p = 2 layer behind it
#   c  5 x 5, k = 2; 60 -> 70 (N over 64) with k = 1, p = 2 giving a 1 x 1 output, then k = 1, p = 1; D = 20; no scalar
#   d  three input channels; k = 5 without a pool; 30 -> 40 with k = 4 (K = 480)
SMALL = {
    'a': (ViewNetSpec(4, ((20, 5, 2), (30, 5, 2)), 30 * 3 * 2 * 6, (16,), 5, 2, 'relu', name='a'), 3, 23, 37, 3),
    'b': (ViewNetSpec(1, ((30, 4, 2), (40, 1, 2)), 40 * 1 * 2 * 1, (12,), 4, 1, 'leaky_relu', name='b'), 1, 12, 9, 5),
    'c': (ViewNetSpec(4, ((60, 2, 2), (70, 1, 2), (70, 1, 1)), 70 * 20, (24, 12), 3, 0, 'relu', name='c'), 20, 5, 5, 2),
    'd': (ViewNetSpec(3, ((30, 5, 1), (40, 4, 2)), 40 * 3 * 2 * 1, (10,), 2, 2, 'relu', name='d'), 3, 12, 9, 2),
}
CMN = (CELLTYPE_CMN(7, 2), 20, 128, 256, 2)      # the smallest H x W this net takes in H: 128 -> ... -> 1


@functools.lru_cache(maxsize=None)
def inputs(name: str, mode: str = 'shapes'):
    """(spec, D, H, W, arrs, views uint8 (n, C, D, H, W), scalars (n, n_scalar) float32) of a case, seeded."""
    spec, D, H, W, n = CMN if name == 'cmn' else SMALL[name]
    seed = 100 + sum(map(ord, name))
    arrs = R.make_weights(spec, seed, D, H, W)
    views = R.synthetic_views(seed + 7, n, spec.in_channels, D, H, W, mode)
    rng = np.random.default_rng(seed + 9)
    scalars = rng.uniform(-1, 1, (n, spec.n_scalar)).astype(np.float32)
    if spec.n_scalar:
        scalars[0, 0] = -1.0      # "no synapses"
    return spec, D, H, W, arrs, views, scalars


# Measured by tests/test_viewnet_cpu.py::test_accumulation_constant over every op of the cases a, b, c, d (modes shapes, zeros, ones,
# checker for a) and cmn, on the stored inputs the float64 chain produces: the largest |ref32 - ref64| / (2^-24 S) of any op, ref32 the
# same op in float32 with torch-CPU (1 and 16 threads gave the same maxima).  Both are set by cmn (f16: a 3.40, c 3.15; bf16: b 2.14).
# c = 4 c_ref, the project's margin for a different summation tree (tests/_unet_step_ref.py), of the measured value itself.
C_REF = {'f16': 4.873, 'bf16': 2.632}
C = {k: 4.0 * v for k, v in C_REF.items()}

# CMN geometry: the device's logits are compared with the float32 restatement ON THE WEIGHTS THE PLAN STORES (R.forward32_stored: the
# convolution weights rounded to the storage type, as StepRef takes them), so that T covers the rounding of the activations only:
# T = 4 x the largest |emulation - float32 restatement| over the two samples of inputs('cmn'), the emulation being that restatement with
# the activations rounded to the storage type behind every layer (R.forward_emul), both on torch-CPU.  Measured by
# tests/test_viewnet_cpu.py::test_cmn_tolerance_and_safety, which recomputes it (1 thread: 0.003533721 / 0.02273196; 16 threads:
# 0.0035289526 / 0.022732198; recorded: the smaller).  The float32 top-2 margins of the two samples are 0.86 and 1.63 (f16 weights) and
# 0.89 and 1.64 (bf16 weights).
EMUL_DIFF = {'f16': 0.0035289526, 'bf16': 0.02273196}
T = {k: 4.0 * v for k, v in EMUL_DIFF.items()}      # 0.0141 / 0.0909


# -- the golden of the reference's own functions (tests/golden/make_golden_celltype.py -> g29_celltype.npz) -----------------------------
# (name, locations, views per location, synapses): one sample with a dropped remainder; the padding branch; one location; three samples
GOLDEN_CELLS = [('c0', 13, 2, 9), ('c1', 3, 2, 0), ('c2', 1, 2, 4), ('c3', 31, 2, 12)]
GOLDEN_WEIGHT_SEED = 290


def golden_cell_inputs(name, n_loc, vpl, n_syn):
    """The generated inputs of a golden cell: views uint8 (n_loc, 4, vpl, 128, 256) and (syn_sign, mesh_area, compartment label)."""
    seed = 2900 + sum(map(ord, name))
    views = R.synthetic_views(seed, n_loc, 4, vpl, 128, 256)
    rng = np.random.default_rng(seed)
    return views, (rng.choice([-1, 1], n_syn), rng.uniform(0.2, 3.0, n_syn), rng.integers(0, 5, n_syn))


@functools.lru_cache(maxsize=None)
def golden_weights():
    return R.make_weights(CELLTYPE_CMN(7, 2), GOLDEN_WEIGHT_SEED, 20, 128, 256)


def crc(*arrays):
    c = 0
    for a in arrays:
        c = zlib.crc32(np.ascontiguousarray(a).tobytes(), c)
    return np.uint32(c)
