"""The representation network of the morphology embedding restated for the tests (torch-CPU / numpy; no kernel code), on top of
tests/_viewnet_ref.py: the module of /root/reference/syconn/cnn/cnn_atn.py:21-55 is ``Conv2d -> MaxPool2d -> act`` on (N, C, H, W), which
is the view net of _viewnet_ref.py on (N, C, 1, H, W) -- a Conv3d with a (1, k, k) kernel and a (1, p, p) pool on a depth of one computes
the same sums --, so the float32 restatement, the emulation with rounded activations and the float64 one-op reference are those,
called with the 5-D twin of the spec.  What is added here: the weights in the module's own 4-D form and key names, drawn so that the
convolution weights are exact in both storage types, and the nearest-location rule of the node mapping in float64.

The reference's flow (reps/super_segmentation_helper.py:1758-1817): ``latent = rep_net(views[:, :, 0] / 255 - 0.5)``; every skeleton
node takes the latent of the rendering location nearest to ``node * scaling`` (``cKDTree.query(k=1)``)."""
import dataclasses

import numpy as np
import torch

import _viewnet_ref as R

# the indices of the Conv2d / Linear modules inside RepresentationNetwork.conv / .fc (cnn_atn.py:32-47, dropout layers included)
CONV_IDX = (0, 3, 6, 9, 13, 17, 20)
FC_IDX = (0, 2)


def spec5(spec):
    """The same net with Conv3d-shaped weights: what _viewnet_ref.py's functions take."""
    return dataclasses.replace(spec, conv_ndim=3)


def make_weights(spec, seed: int, H: int, W: int, exact: bool = True):
    """[w, b, ...] float32, convolution weights 5-D (cout, cin, 1, k, k) as _viewnet_ref.py wants them.  `exact`: the convolution
    weights rounded to bfloat16 with values below 2^-14 flushed to zero, so that they are the same numbers in fp16, bf16 and float32
    and the plan stores exactly what the float32 module computes with."""
    arrs = R.make_weights(spec5(spec), seed, 1, H, W)
    if exact:
        for i in range(len(spec.layers)):
            w = torch.from_numpy(arrs[2 * i]).to(torch.bfloat16).float()
            w[w.abs() < 2.0 ** -14] = 0.0
            assert torch.equal(w.to(torch.float16).float(), w)
            arrs[2 * i] = w.numpy()
    return arrs


def state_dict_of(spec, arrs, prefix: str = '', ndim: int = 2):
    """The state dict of the bare module (``conv.N.*``, ``fc.N.*``) or, with ``prefix='rep_net.'``, of the whole TripletNet; `ndim` 2:
    Conv2d weights (cout, cin, k, k), 3: Conv3d ones."""
    nl, out = len(spec.layers), {}
    conv_idx = CONV_IDX if nl == len(CONV_IDX) else tuple(range(0, 3 * nl, 3))
    for i in range(nl):
        w = torch.from_numpy(arrs[2 * i])
        out[f'{prefix}conv.{conv_idx[i]}.weight'] = w[:, :, 0] if ndim == 2 else w
        out[f'{prefix}conv.{conv_idx[i]}.bias'] = torch.from_numpy(arrs[2 * i + 1])
    for j in range(len(spec.linear_sizes) - 1):
        out[f'{prefix}fc.{2 * j}.weight'] = torch.from_numpy(arrs[2 * nl + 2 * j])
        out[f'{prefix}fc.{2 * j}.bias'] = torch.from_numpy(arrs[2 * nl + 2 * j + 1])
    return out


def _views5(views_u8):
    v = np.asarray(views_u8)
    return np.ascontiguousarray(v[:, :, None] if v.ndim == 4 else v[:, :, :1])


def latent32(spec, arrs, views_u8, store=None, dtype=torch.float32):
    """The float32 (or float64) restatement: uint8 views (n, C, H, W), or (n_loc, C, nb_views, H, W) of which view 0 is taken ->
    latents (n, z).  `store`: convolution weights as the plan stores them."""
    return R.forward32(spec5(spec), arrs, _views5(views_u8), None, weights_as=store, dtype=dtype)


def latent_emul(spec, arrs, views_u8, store):
    """latent32 on the stored weights with the activations rounded to the storage type behind every layer."""
    return R.forward32(spec5(spec), arrs, _views5(views_u8), None, store=store, weights_as=store)


def nearest_rows(locations, queries):
    """For every float64 query the row of the nearest location, distances ((dx dx) + dy dy) + dz dz in float64, the smaller row on
    equal distances; and whether the two smallest distances of the query are equal (a tie)."""
    loc = np.asarray(locations, dtype=np.float64).reshape(-1, 3)
    q = np.asarray(queries, dtype=np.float64).reshape(-1, 3)
    d = loc[None] - q[:, None]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    rows = np.argmin(d2, axis=1)
    s = np.sort(d2, axis=1)
    tie = s[:, 0] == s[:, 1] if loc.shape[0] > 1 else np.zeros(len(q), bool)
    return rows.astype(np.int64), tie
