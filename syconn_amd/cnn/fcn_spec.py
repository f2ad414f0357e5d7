"""The 2D semantic-segmentation networks of the compartment step as a spec: a VGG-style encoder of five blocks and the FCN decoder of
five stride-2 transposed convolutions with skip additions.

The reference builds them as ``FCNs(base_net=VGGNet(model='vgg13', in_channels=4), n_class=5 | 6)``
(/root/reference/syconn/cnn/cnn_spineseg.py:28-29, cnn_axonseg.py:34-35) from ``elektronn3.models.fcn_2d``, which is not part of the
reference tree.  Everything below about the architecture is therefore **stated, not pinned**:

* Encoder (VGG13 ``features``, no normalisation): five blocks of ``[Conv2d(3x3, padding=1) + ReLU] x 2`` followed by
  ``MaxPool2d(2, 2)``; channels 64, 128, 256, 512, 512; ``x1 ... x5`` are the five pooled outputs.
* Decoder: ``score = bn_i(relu(deconv_i(score)))``, then ``score = score + x_{5-i}`` for i = 1..4; every ``deconv_i`` is
  ``ConvTranspose2d(k=3, stride=2, padding=1, output_padding=1)`` (its output is exactly 2x its input); channels 512 -> 512, 512 -> 256,
  256 -> 128, 128 -> 64, 64 -> 32; ``bn_i`` is an eval-mode BatchNorm2d applied AFTER the ReLU, so it cannot be folded into the
  deconvolution's weights; then ``Conv2d(32, n_class, 1)``.
* Input: ``views.astype(float32) / 255.`` without ``- 0.5`` (reps/super_segmentation_helper.py:1372; ``get_semseg_*_model`` pass no
  ``normalize_func``).
* Label: ``np.argmax(., axis=1)``: the first maximum wins a tie.  Whether ``InferenceModel.predict_proba`` applies a softmax is not in
  the tree and does not change the argmax.
* Geometry: H and W must be multiples of 32, otherwise the skip additions do not fit; anything else is a ValueError.
"""
from collections import OrderedDict
from dataclasses import dataclass, field
from typing import List, Tuple

import numpy as np

BN_EPS = 1e-5


@dataclass(frozen=True)
class FcnSpec:
    in_channels: int
    blocks: Tuple[Tuple[int, ...], ...]      # output channels of the convolutions of each of the five blocks
    dec_last: int                            # output channels of the fifth transposed convolution
    n_class: int
    name: str = field(default='fcn', compare=False)

    def __post_init__(self):
        object.__setattr__(self, 'blocks', tuple(tuple(int(c) for c in b) for b in self.blocks))
        if not 1 <= self.in_channels <= 4:
            raise ValueError('in_channels must be 1 to 4 (the renderer writes at most four channels)')
        if len(self.blocks) != 5:
            raise ValueError('an FCN has exactly five encoder blocks')
        for i, b in enumerate(self.blocks):
            if not 1 <= len(b) <= 3:
                raise ValueError(f'block {i}: 1 to 3 convolutions, got {len(b)}')
            if any(not 1 <= c <= 512 for c in b):
                raise ValueError(f'block {i}: channels must be 1 ... 512')
        if not 1 <= self.dec_last <= 512:
            raise ValueError('dec_last must be 1 ... 512')
        if not 1 <= self.n_class <= 16:
            raise ValueError('n_class must be 1 ... 16')

    # -- structure ------------------------------------------------------------------------------------------------------------
    @property
    def convs(self) -> List[Tuple[int, int, int, bool]]:
        """(block, cin, cout, pooled) of every encoder convolution in order; `pooled`: the block's last one (its 2 x 2 pool is fused)."""
        out, cin = [], self.in_channels
        for bi, b in enumerate(self.blocks):
            for j, c in enumerate(b):
                out.append((bi, cin, c, j == len(b) - 1))
                cin = c
        return out

    @property
    def deconvs(self) -> List[Tuple[int, int]]:
        """(cin, cout) of the five transposed convolutions: the outputs are the channels of x4, x3, x2, x1, then dec_last."""
        x = [b[-1] for b in self.blocks]
        outs = [x[3], x[2], x[1], x[0], self.dec_last]
        return list(zip([x[4]] + outs[:-1], outs))

    @property
    def n_ops(self) -> int:
        return len(self.convs) + 5 + 1

    def check_geometry(self, H: int, W: int) -> None:
        if H < 32 or W < 32 or H % 32 or W % 32:
            raise ValueError(f'{self.name}: H and W must be positive multiples of 32 (the skip additions do not fit otherwise), got {H} x {W}')

    def shapes(self, H: int, W: int) -> List[Tuple[int, int, int]]:
        """(channels, h, w) of every stored tensor in op order: the encoder convolutions (the last of a block behind its pool), the five
        decoder steps, the classifier's logits."""
        self.check_geometry(H, W)
        out = []
        for bi, _, cout, pooled in self.convs:
            s = bi + 1 if pooled else bi
            out.append((cout, H >> s, W >> s))
        for i, (_, cout) in enumerate(self.deconvs):
            out.append((cout, H >> (4 - i), W >> (4 - i)))
        out.append((self.n_class, H, W))
        return out

    def param_shapes(self) -> 'OrderedDict[str, tuple]':
        """Registration order of ``FCNs(VGGNet)``: the encoder's ``features`` (index = position in the Sequential with its ReLU and
        MaxPool entries), ``deconv_i`` / ``bn_i`` pairs, the classifier."""
        out, pos = OrderedDict(), 0
        for _, cin, cout, pooled in self.convs:
            out[f'pretrained_net.features.{pos}.weight'] = (cout, cin, 3, 3)
            out[f'pretrained_net.features.{pos}.bias'] = (cout,)
            pos += 3 if pooled else 2
        for i, (cin, cout) in enumerate(self.deconvs, 1):
            out[f'deconv{i}.weight'] = (cin, cout, 3, 3)
            out[f'deconv{i}.bias'] = (cout,)
            for nm in ('weight', 'bias', 'running_mean', 'running_var'):
                out[f'bn{i}.{nm}'] = (cout,)
        out['classifier.weight'] = (self.n_class, self.dec_last, 1, 1)
        out['classifier.bias'] = (self.n_class,)
        return out

    def macs_per_view(self, H: int, W: int) -> int:
        """Multiply-adds of one H x W view over real channels: convolutions 9 cin cout per output pixel before the pool, transposed
        convolutions 9 cin cout per INPUT pixel (every input pixel meets every tap once; the taps that would read past the high edge
        are counted, they multiply zeros), the classifier dec_last n_class per pixel."""
        self.check_geometry(H, W)
        macs = 0
        for bi, cin, cout, _ in self.convs:
            macs += (H >> bi) * (W >> bi) * 9 * cin * cout
        for i, (cin, cout) in enumerate(self.deconvs):
            macs += (H >> (5 - i)) * (W >> (5 - i)) * 9 * cin * cout
        return macs + H * W * self.dec_last * self.n_class

    # -- weights --------------------------------------------------------------------------------------------------------------
    def weights_from_state_dict(self, state_dict) -> List[np.ndarray]:
        """The float32 arrays of ``param_shapes()`` from a state dict in registration order, whatever its keys are called: tensors are
        matched by shape and role in order -- 4-D (cout, cin, 3, 3) encoder weights, 4-D (cin, cout, 3, 3) transposed-convolution
        weights, four 1-D BatchNorm tensors per step --; 0-d entries (``num_batches_tracked``) are skipped.  Any other extra tensor, a
        wrong shape or a non-finite value raises."""
        arrs = []
        for k, v in state_dict.items():
            a = v.detach().cpu().numpy() if hasattr(v, 'detach') else np.asarray(v)
            if a.ndim == 0:
                continue
            arrs.append((k, np.ascontiguousarray(a, dtype=np.float32)))
        want = list(self.param_shapes().items())
        if len(arrs) != len(want):
            raise ValueError(f'{self.name}: the state dict has {len(arrs)} tensors (0-d entries not counted), the spec needs {len(want)}')
        for (key, a), (name, shape) in zip(arrs, want):
            if tuple(a.shape) != tuple(shape):
                raise ValueError(f'{self.name}: {key} has shape {tuple(a.shape)}, the spec needs {tuple(shape)} ({name})')
            if not np.isfinite(a).all():
                raise ValueError(f'{self.name}: {key} holds non-finite values')
        return [a for _, a in arrs]


def FCN_VGG13(n_class: int, in_channels: int = 4) -> FcnSpec:
    """cnn_spineseg.py:28-29 (n_class 5) / cnn_axonseg.py:34-35 (n_class 6)."""
    return FcnSpec(in_channels, ((64, 64), (128, 128), (256, 256), (512, 512), (512, 512)), 32, n_class, name='fcn_vgg13')
