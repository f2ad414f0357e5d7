"""Bit digest of the 2D view networks (csrc/sd_viewnet.hip, csrc/sd_fcn.hip): seeded nets on seeded uint8 views in both storage types,
one line per stored tensor with the sha256 of its bytes -- every layer / op / Linear through ``read_buffer``, the logits and the
labels.  Two builds of the library compute the same bits exactly if their outputs are the same text.

    python tools/viewnets_digest.py [--out profiles/viewnets_digest.txt]

The cases are the smallest that reach every branch of the planar layer core (csrc/sd_planar_mma.h):

* view net: 3 channels, layers (13, k 5, pool 2), (70, k 1, pool 1), (10, k 4, pool 2) -- one and five N tiles -- on 30 x 46 views (26 x 42
  and 13 x 21 outputs: several tiles, partial ones along both axes), D = 3, 11 samples whose table draws planes in any order, two
  scalars; the plain head and the sample-tiled one (8 + 3 samples: a partial last tile);
* FCN ``a``: 3 channels, blocks (12, 72), (24), (40, 40), (72), (72): a first layer without a pool, two channel groups, two chunks; FCN
  ``b``: 1 channel, blocks (8), (16), (24), (40), (40): a first layer with its pool fused; three planes of 32 x 64 in launch sets of two,
  so the last one starts at plane 2; transposed convolutions with and without a skip; logits kept (``predict_proba``) and not
  (``predict_labels``)."""
import argparse
import hashlib
import os
import sys
from collections import OrderedDict

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def state_dict(spec, seed):
    """Seeded weights in the spec's registration order: He-scaled weights, small biases, BatchNorm scales and variances in 0.5 ... 1.5."""
    rng = np.random.default_rng(seed)
    out = OrderedDict()
    for name, shape in spec.param_shapes().items():
        if len(shape) > 1:
            a = rng.standard_normal(shape) * np.sqrt(2. / np.prod(shape[1:]))
        elif name.startswith('bn') and name.endswith(('weight', 'running_var')):
            a = rng.uniform(0.5, 1.5, shape)
        else:
            a = rng.standard_normal(shape) * 0.1
        out[name] = a.astype(np.float32)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    from syconn_amd.cnn.fcn_spec import FcnSpec
    from syconn_amd.cnn.viewnet_spec import ViewNetSpec
    from syconn_amd.handler.prediction import EmbeddingModel, SemsegViewModel, ViewModel, ViewSamples
    lines = []

    def put(case, store, name, a):
        a = np.ascontiguousarray(a.cpu().numpy() if isinstance(a, torch.Tensor) else a)
        lines.append(f'{case} {store} {name} {a.dtype} {"x".join(str(s) for s in a.shape)} {hashlib.sha256(a.tobytes()).hexdigest()}')

    rng = np.random.default_rng(7)
    vspec = ViewNetSpec(3, ((13, 5, 2), (70, 1, 1), (10, 4, 2)), 10 * 3 * 5 * 9, (50, 30), 4, 2, 'relu', name='digest')
    n_loc, nb_views, D, H, W, n = 5, 4, 3, 30, 46, 11
    views = rng.integers(0, 256, (n_loc, 3, nb_views, H, W), dtype=np.uint8)
    table = rng.integers(0, n_loc * nb_views, (n, D)).astype(np.int32)
    scal = rng.uniform(0, 1, (n, 2)).astype(np.float32)
    vsd = state_dict(vspec, 1)
    fcns = (('fcn_a', FcnSpec(3, ((12, 72), (24,), (40, 40), (72,), (72,)), 20, 5, name='a'), 2),
            ('fcn_b', FcnSpec(1, ((8,), (16,), (24,), (40,), (40,)), 12, 3, name='b'), 3))
    for store in ('f16', 'bf16'):
        for case, cls, run in (('viewnet', ViewModel, 'predict_proba'), ('viewnet_tiled', EmbeddingModel, 'forward_samples')):
            m = cls(vspec, vsd, act_dtype=store, bs=16, device='cuda:0')
            put(case, store, 'logits', getattr(m, run)((ViewSamples(views, table), scal)))
            for i in range(m.num_ops):
                put(case, store, f'buffer{i}', m.read_buffer(i))
        for case, spec, seed in fcns:
            fv = rng.integers(0, 256, (3, spec.in_channels, 32, 64), dtype=np.uint8)
            m = SemsegViewModel(spec, state_dict(spec, seed), act_dtype=store, bs=2, device='cuda:0')
            put(case, store, 'logits', m.predict_proba(fv))
            for i in range(m.num_ops):
                put(case, store, f'buffer{i}', m.read_buffer(i))
            put(case, store, 'labels', m.predict_labels(fv[:, :, None]))
            put(case, store, 'labels_buffer0', m.read_buffer(0))
    text = '\n'.join(lines) + '\n'
    sys.stdout.write(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
