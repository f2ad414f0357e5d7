"""Golden vectors for the pixel labels of the compartment step, produced by the REFERENCE'S OWN ``predict_views_semseg``
(/root/reference/syconn/reps/super_segmentation_helper.py:1353-1392), lifted by AST at generation time and run unchanged on numpy with a
torch-CPU float32 model.  Nothing compiled and no reference text is stored: label outputs only, and a CRC of the generated inputs and
weights, so that a drift of the generators of tests/_fcn_ref.py shows as itself.

    python tests/golden/make_golden_semseg.py      ->  tests/golden/g30_semseg.npz

Stated stand-ins (not reference code): ``FCNs(VGGNet)`` of elektronn3 = ``_fcn_ref.Fcns`` (syconn_amd/cnn/fcn_spec.py says what is stated
about it); ``InferenceModel.predict_proba`` = the module in eval mode on float32 tensors, without a softmax (it would not change the
argmax)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import _fcn_cases as K  # noqa: E402
import _fcn_ref as R  # noqa: E402
from make_golden_cs import lift_function  # noqa: E402

REF = '/root/reference/syconn'


def main():
    ns = {'np': np}
    lift_function(f'{REF}/reps/super_segmentation_helper.py', 'predict_views_semseg', ns)
    out = {'names': np.array([g[0] for g in K.GOLDEN])}
    for name, _, n_loc, nb_views in K.GOLDEN:
        spec, arrs, views = K.golden_inputs(name)
        net = R.Fcns(spec).eval()
        net.load_state_dict({**net.state_dict(), **R.state_dict_of(spec, arrs)})

        class Model:
            def predict_proba(self, inp, bs=10, verbose=False):
                assert inp.dtype == np.float32 and inp.shape[1] == spec.in_channels
                with torch.no_grad():
                    return net(torch.from_numpy(np.ascontiguousarray(inp))).numpy()

        labels = ns['predict_views_semseg'](views.copy(), Model(), batch_size=10)
        assert labels.shape == (n_loc, 1, nb_views) + views.shape[3:] and 0 <= labels.min() and labels.max() < spec.n_class
        out.update({f'{name}_crc': K.crc(views, *arrs), f'{name}_labels': labels.astype(np.uint8)})
        print(name, labels.shape, np.bincount(labels.ravel(), minlength=spec.n_class))
    path = os.path.join(HERE, 'g30_semseg.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes;', len(out), 'arrays')


if __name__ == '__main__':
    main()
