"""The multi-view networks as a spec: planar layers "valid k x k convolution, (1, p, p) floor max-pool, activation" followed by a
chain of Linear layers over ``[x.view(N, -1), scalars]``.

The reference writes this architecture down as ``StackedConv2ScalarWithLatentAdd``
(/root/reference/syconn/cnn/cnn_celltype_cmn_j0251.py:22-60, cnn_celltype_cmn.py:21-57) on elektronn3's ``Conv3DLayer``, which is
not part of the reference tree.  What the tree pins about that layer: the in-tree comment "given (1, 4, 20, 128, 256)" and the
``4200`` inputs of the first Linear only work out for a convolution without padding followed by a floor-mode pool
(128 x 256 -> 62 x 126 -> 29 x 61 -> 13 x 29 -> 5 x 13 -> 2 x 6 -> 1 x 3 -> 1 x 3; 70 * 20 * 1 * 3 = 4200).  What is stated, not
pinned: no normalisation layer inside ``Conv3DLayer`` (the in-tree calls pass none) and the pool before the activation (the order
changes no value: a maximum commutes with a rising map).  Dropout is the identity in inference.
"""
from collections import OrderedDict
from dataclasses import dataclass, field
from typing import List, Tuple

import numpy as np

KERNELS = (1, 2, 4, 5)
ACTS = ('relu', 'leaky_relu')


@dataclass(frozen=True)
class ViewNetSpec:
    in_channels: int
    layers: Tuple[Tuple[int, int, int], ...]      # (cout, k, pool)
    fc_in: int                                    # flattened features the first Linear takes (without the scalars)
    fc: Tuple[int, ...]                           # hidden sizes h1, h2, ...
    n_classes: int
    n_scalar: int = 0
    act: str = 'relu'
    name: str = field(default='viewnet', compare=False)
    conv_ndim: int = 3                            # 3: Conv3d weights (cout, cin, 1, k, k); 2: Conv2d weights (cout, cin, k, k)

    def __post_init__(self):
        object.__setattr__(self, 'layers', tuple(tuple(int(v) for v in l) for l in self.layers))
        object.__setattr__(self, 'fc', tuple(int(v) for v in self.fc))
        if self.act not in ACTS:
            raise ValueError(f'act must be one of {ACTS}, got {self.act!r}')
        if self.conv_ndim not in (2, 3):
            raise ValueError('conv_ndim must be 2 (Conv2d weights) or 3 (Conv3d weights)')
        if not 1 <= self.in_channels <= 4:
            raise ValueError('in_channels must be 1 to 4 (the renderer writes at most four channels)')
        if not self.layers:
            raise ValueError('a view net has at least one layer')
        for i, (cout, k, pool) in enumerate(self.layers):
            if k not in KERNELS:
                raise ValueError(f'layer {i}: k = {k} is not one of {KERNELS}')
            if pool not in (1, 2):
                raise ValueError(f'layer {i}: pool = {pool} is not 1 or 2')
            if not 1 <= cout <= 80:
                raise ValueError(f'layer {i}: cout = {cout} is not in 1 ... 80')
        if self.n_scalar < 0 or self.n_classes < 1 or self.fc_in < 1 or any(h < 1 for h in self.fc) or len(self.fc) > 3:
            raise ValueError('bad head: fc_in, n_classes >= 1, n_scalar >= 0, at most three hidden Linear layers')

    # -- shapes ---------------------------------------------------------------------------------------------------------------
    def layer_shapes(self, H: int, W: int) -> List[Tuple[int, int]]:
        """(Ho, Wo) behind every layer: valid convolution, floor pool.  ValueError where a layer's output would be empty."""
        out, h, w = [], int(H), int(W)
        for i, (_, k, pool) in enumerate(self.layers):
            h, w = max(h - k + 1, 0) // pool, max(w - k + 1, 0) // pool
            if h < 1 or w < 1:
                raise ValueError(f'layer {i} has an empty output for a {H} x {W} view')
            out.append((h, w))
        return out

    def check_geometry(self, D: int, H: int, W: int) -> List[Tuple[int, int]]:
        """layer_shapes, and ValueError if the flattened size is not what the first Linear takes."""
        if D < 1:
            raise ValueError('D must be positive')
        shapes = self.layer_shapes(H, W)
        flat = self.layers[-1][0] * D * shapes[-1][0] * shapes[-1][1]
        if flat != self.fc_in:
            raise ValueError(f'{self.name}: a ({D}, {H}, {W}) sample flattens to {flat} features, the first Linear takes {self.fc_in}')
        return shapes

    @property
    def linear_sizes(self) -> Tuple[int, ...]:
        """Inputs of the first Linear, then the outputs of every Linear."""
        return (self.fc_in + self.n_scalar,) + self.fc + (self.n_classes,)

    def param_shapes(self) -> 'OrderedDict[str, tuple]':
        """Registration order of the reference's module: convolution weights (5-D, or 4-D with ``conv_ndim = 2``) and biases, then the
        Linear ones."""
        out, cin = OrderedDict(), self.in_channels
        for i, (cout, k, _) in enumerate(self.layers):
            out[f'seq.{i}.conv.weight'] = (cout, cin, 1, k, k) if self.conv_ndim == 3 else (cout, cin, k, k)
            out[f'seq.{i}.conv.bias'] = (cout,)
            cin = cout
        sizes = self.linear_sizes
        for j in range(len(sizes) - 1):
            out[f'fc.{2 * j}.weight'] = (sizes[j + 1], sizes[j])
            out[f'fc.{2 * j}.bias'] = (sizes[j + 1],)
        return out

    def macs_per_sample(self, D: int, H: int, W: int) -> int:
        """Multiply-adds of one sample: every convolution output that a pool window keeps (rows and columns the floor pool drops are
        never computed), real channels only, plus the head."""
        shapes, cin, macs = self.check_geometry(D, H, W), self.in_channels, 0
        for (cout, k, pool), (h, w) in zip(self.layers, shapes):
            macs += D * (h * pool) * (w * pool) * k * k * cin * cout
            cin = cout
        sizes = self.linear_sizes
        return macs + sum(a * b for a, b in zip(sizes[:-1], sizes[1:]))

    def flops_per_sample(self, D: int, H: int, W: int) -> int:
        return 2 * self.macs_per_sample(D, H, W)

    # -- weights --------------------------------------------------------------------------------------------------------------
    def weights_from_state_dict(self, state_dict) -> List[np.ndarray]:
        """The float32 arrays [w, b, w, b, ...] of the spec from a state dict in registration order, whatever its keys are called
        (so a ``torch.jit.load``-ed module works, and a module wrapped in another one): the 5-D tensors (4-D for a ``conv_ndim = 2``
        spec) are the convolution weights, the 2-D ones the Linear weights, each followed by its 1-D bias.  Every shape is checked against the spec; other entries (none in the reference's module) raise."""
        arrs = [(k, np.ascontiguousarray(v.detach().cpu().numpy() if hasattr(v, 'detach') else np.asarray(v), dtype=np.float32))
                for k, v in state_dict.items()]
        want = list(self.param_shapes().items())
        if len(arrs) != len(want):
            raise ValueError(f'{self.name}: the state dict has {len(arrs)} tensors, the spec needs {len(want)}')
        for (key, a), (name, shape) in zip(arrs, want):
            if tuple(a.shape) != tuple(shape):
                raise ValueError(f'{self.name}: {key} has shape {tuple(a.shape)}, the spec needs {tuple(shape)} ({name})')
            if not np.isfinite(a).all():
                raise ValueError(f'{self.name}: {key} holds non-finite values')
        return [a for _, a in arrs]


def CELLTYPE_CMN(n_classes: int = 7, n_scalar: int = 2, act: str = 'relu', in_channels: int = 4) -> ViewNetSpec:
    """cnn_celltype_cmn_j0251.py:22-60 for 20 views of 128 x 256."""
    return ViewNetSpec(in_channels, ((20, 5, 2), (30, 5, 2), (40, 4, 2), (50, 4, 2), (60, 2, 2), (70, 1, 2), (70, 1, 1)), 4200,
                       (100, 50), n_classes, n_scalar, act, name='celltype_cmn')


def VIEWNET_SMALL(n_classes: int = 2, n_scalar: int = 0, act: str = 'relu', in_channels: int = 4) -> ViewNetSpec:
    """The commented-out family of cnn_celltype_cmn.py:60-95 (13, 19, 25, 25, 30, 30, 31; 1860 + n -> 50 -> 30 -> n), also the
    convolution stack of the glia view model."""
    return ViewNetSpec(in_channels, ((13, 5, 2), (19, 5, 2), (25, 4, 2), (25, 4, 2), (30, 2, 2), (30, 1, 2), (31, 1, 1)), 1860,
                       (50, 30), n_classes, n_scalar, act, name='viewnet_small')


def GLIA_CMN(n_classes: int = 2, act: str = 'relu') -> ViewNetSpec:
    """The glia view model, ``StackedConv2Scalar(1, 2)`` of cnn_gliaviews_e3.py:27 (``get_model``) behind ``get_glia_model_e3``
    (handler/prediction.py:978-982).  ``elektronn3.models.simple`` is not part of the reference tree.  Pinned by the tree: one input
    channel (the raw views only: ``raw_only=True`` in ``predict_views_gliaSV``) and two classes (``StackedConv2Scalar(1, 2)``), 2 views
    per sample (``nb_views: 2`` in cnn_gliaviews_e3.py), no scalars, ``naive_view_normalization_new`` as the normalisation.  Stated, not
    pinned: the layer widths, which are the ``VIEWNET_SMALL`` stack, the commented family of cnn_celltype_cmn.py:60-95 -- 2 views of
    128 x 256 flatten to 31 x 2 x 1 x 3 = 186 features, then 186 -> 50 -> 30 -> 2 --, and the softmax behind the logits
    (``GliaViewModel``)."""
    s = VIEWNET_SMALL(n_classes, 0, act, in_channels=1)
    return ViewNetSpec(1, s.layers, 186, s.fc, n_classes, 0, act, name='glia_cmn')


def TNET_REP(z_dim: int = 25, fc_in: int = 372, in_channels: int = 4) -> ViewNetSpec:
    """``RepresentationNetwork`` of cnn_atn.py:21-55 as ``get_model`` builds it (:111-116, ReLU; Dropout2d is the identity in
    inference): Conv2d 13 (5, pool) / 19 (5, pool) / 25 (4) / 25 (4, pool) / 30 (2, pool) / 30 (2, pool) / 31 (1), then
    Linear(fc_in, 50) -> ReLU -> Linear(50, z_dim) on single views (D = 1).  ``fc_in = 372`` is what the 128 x 256 window of the config
    flattens to (31 x 2 x 6) and what the tree's commented ``Linear(372, 50)`` takes; the module as written has ``Linear(6076, 50)``,
    and 6076 = 31 x 14 x 14 is what a 512 x 512 view flattens to: 512 -> 508 -> 254 -> 250 -> 125 -> 122 -> 119 -> 59 -> 58 -> 29 -> 28 ->
    14.  The smallest view the stack takes is 92 x 92 (31 features).  Weights are ``Conv2d`` ones (``conv_ndim = 2``): the state dict
    of the bare module (``conv.N.*``, ``fc.N.*``) and of the whole ``TripletNet`` (``rep_net.*``) load alike, by registration order."""
    return ViewNetSpec(in_channels, ((13, 5, 2), (19, 5, 2), (25, 4, 1), (25, 4, 2), (30, 2, 2), (30, 2, 2), (31, 1, 1)), fc_in, (50,), z_dim,
                       0, 'relu', name='tnet_rep', conv_ndim=2)
