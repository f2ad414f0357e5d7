"""The cases of the FCN tests (tests/test_fcn_cpu.py, tests/test_gpu_fcn.py) and the constants measured on them."""
import functools

import numpy as np

from syconn_amd.cnn.fcn_spec import FCN_VGG13, FcnSpec

import _fcn_ref as R

STORES = ('f16', 'bf16')

S_NET = FcnSpec(3, ((12, 20), (24,), (40, 40, 40), (72, 72), (72,)), 20, 5, name='s')


def _o_net(n_class):
    return FcnSpec(1, ((8,), (16,), (24,), (40,), (40,)), 12, n_class, name=f'o{n_class}')


# name -> (spec, n_loc, nb_views, H, W).  The smallest shapes at which each path can go wrong:
#   v   the real channel counts (K = 4608, N = 512) at 32 x 64, 2 locations x 2 views: x5 is 1 x 2, every deep layer is smaller than a
#       tile and the transposed convolution's zero edge is half its input
#   s   widths 96, 48, 24, 12, 6, 3: partial tiles at every level; channels no multiple of 8 / 16 / 32 (72: two channel groups of three N
#       tiles); blocks of 1 and 3 convolutions; 3 planes; the first layer is not pool-fused
#   o1, o2  one input channel, blocks of one convolution: the first layer is uint8 AND pool-fused; x5 is 1 x 1; n_class 1 and 2
#   w   the s net at 32 x 1024: many tiles along x
#   g   the spiness geometry itself: FCN_VGG13(5) at 128 x 256, 1 location x 2 views
CASES = {
    'v': (FCN_VGG13(6), 2, 2, 32, 64),
    's': (S_NET, 3, 1, 64, 96),
    'o1': (_o_net(1), 1, 1, 32, 32),
    'o2': (_o_net(2), 1, 1, 32, 32),
    'w': (S_NET, 1, 1, 32, 1024),
    'g': (FCN_VGG13(5), 1, 2, 128, 256),
}
MODES = ('shapes', 'zeros', 'ones', 'checker')      # the input modes run on s
E2E = ('v', 's', 'g')
SEED = {'v': 318, 's': 215, 'o1': 160, 'o2': 161, 'w': 219, 'g': 303}


@functools.lru_cache(maxsize=None)
def weights(name: str):
    spec, _, _, H, W = CASES[name]
    return R.make_weights(spec, SEED[name], H, W)


@functools.lru_cache(maxsize=None)
def inputs(name: str, mode: str = 'shapes'):
    """(spec, arrs, views uint8 (n_loc, C, nb_views, H, W)) of a case, seeded."""
    spec, n_loc, nb_views, H, W = CASES[name]
    return spec, weights(name), R.synthetic_views(SEED[name] + 7, n_loc, spec.in_channels, nb_views, H, W, mode)


@functools.lru_cache(maxsize=None)
def restatement(name: str, store: str):
    """The float32 restatement's logits of a case on the stored weights (shared by the tests that need it; do not modify)."""
    spec, arrs, views = inputs(name)
    out = R.forward32_stored(spec, arrs, R.planes_of(views), store)
    out.setflags(write=False)
    return out


# Measured by tests/test_fcn_cpu.py::test_accumulation_constant over every op of every case (modes shapes, zeros, ones, checker for s) on
# the stored inputs the float64 chain produces: the largest |ref32 - ref64| / (2^-24 S) of any op, ref32 the same op in float32 with
# torch-CPU.  K = 9 x 512 here is 8 times the view net's, hence re-measured (tests/_viewnet_cases.py: 4.873 / 2.632).
# Both are set by v (f16: g 5.271, s:checker 5.110, s 4.934, w 4.409; bf16: w 3.955, s 3.849, g 3.767; o1 / o2 2.0 - 2.6); 1, 4 and
# all threads gave the same maxima.  c = 4 c_ref, the project's margin for a different summation tree (tests/_unet_step_ref.py).
C_REF = {'f16': 5.613, 'bf16': 4.854}
C = {k: 4.0 * v for k, v in C_REF.items()}

# End to end (v, s, g): the device's logits are compared with the float32 restatement ON THE WEIGHTS THE PLAN STORES, so that T covers
# the rounding of the activations only: T = 4 x the largest |emulation - restatement| of the case, the emulation being the restatement
# with the activations rounded to the storage type behind every stored tensor (R.forward_emul), both on torch-CPU.  Measured by
# tests/test_fcn_cpu.py::test_tolerance_and_left_out, which recomputes them (1, 4 and all threads agree to six digits).  The logits have
# an RMS of 2.0 - 2.1; the emulation's argmax differs from the restatement's at 0.04 - 0.05 % (f16) and 0.30 - 0.36 % (bf16) of the pixels,
# and 32 - 38 % of the pixels have a margin below 2 T in bf16, which is why no end-to-end label comparison is made there.
EMUL_DIFF = {'f16': {'v': 0.008717656, 's': 0.009578943, 'g': 0.01200372}, 'bf16': {'v': 0.07281351, 's': 0.08211613, 'g': 0.09854102}}
T = {st: {k: 4.0 * v for k, v in d.items()} for st, d in EMUL_DIFF.items()}
# the share of pixels whose restatement top-2 margin is below 2 T (left out of the fp16 end-to-end label comparison; at most 10 %)
LEFT_OUT_E2E = {'v': 0.0514, 's': 0.0512, 'g': 0.0450}


# -- the golden of the reference's own predict_views_semseg (tests/golden/make_golden_semseg.py -> g30_semseg.npz) ----------------------
# (name, case whose net and weights it takes, locations, views per location).  The 3 x 3 weights are the case's rounded to bfloat16,
# values below 2^-14 flushed to zero: exact in BOTH storage types, so the plan stores the golden model's own weights and the golden
# labels are the float32 restatement's.
GOLDEN = [('o2', 'o2', 3, 2), ('s', 's', 2, 3)]


@functools.lru_cache(maxsize=None)
def golden_inputs(name: str):
    """(spec, arrs, views uint8 (n_loc, C, nb_views, H, W)) of a golden case."""
    import torch
    _, case, n_loc, nb_views = [g for g in GOLDEN if g[0] == name][0]
    spec, _, _, H, W = CASES[case]
    arrs = []
    for a in weights(case):
        if a.ndim == 4 and a.shape[2:] == (3, 3):
            a = torch.from_numpy(a).to(torch.bfloat16).float().numpy()
            a = np.where(np.abs(a) < 2.0 ** -14, np.float32(0), a)
        arrs.append(a)
    return spec, arrs, R.synthetic_views(3000 + SEED[case], n_loc, spec.in_channels, nb_views, H, W)


def crc(*arrays):
    import zlib
    c = 0
    for a in arrays:
        c = zlib.crc32(np.ascontiguousarray(a).tobytes(), c)
    return np.uint32(c)


# T of the golden cases, as EMUL_DIFF above (tests/test_fcn_cpu.py::test_golden_semseg recomputes them)
GOLDEN_EMUL_DIFF = {'f16': {'o2': 0.009414077, 's': 0.009489059}, 'bf16': {'o2': 0.07280648, 's': 0.09124506}}
GOLDEN_T = {st: {k: 4.0 * v for k, v in d.items()} for st, d in GOLDEN_EMUL_DIFF.items()}
