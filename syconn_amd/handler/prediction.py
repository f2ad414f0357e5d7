"""Drop-in for the dense part of ``syconn.handler.prediction`` (/root/reference/syconn/handler/prediction.py:594-868)
plus the ``elektronn3.inference.Predictor`` subset SyConn uses on this path.

Same names, argument meaning and error behaviour as the reference; the compute underneath is the HIP library
(``include/syconn_dense.h``).  There is no CPU fallback: without the built library / an MI355X every entry point
that needs compute raises.
"""
import itertools
import logging
import os
import shutil
from logging import Logger
from typing import Any, Iterable, Optional, Tuple, Union

import numpy as np
import torch

from .. import _lib as L
from .. import global_params
from ..knossos import ChunkDataset, KnossosDataset
from . import basics
from .basics import chunkify
from .config import initialize_logging

log_main = logging.getLogger('syconn_amd.handler')
log_reps = log_main


# ------------------------------------------------------------------------------------------------------
# axis helpers (prediction.py:279-307)
def xyz2zyx(vol: np.ndarray) -> np.ndarray:
    """[..., X, Y, Z] -> [..., Z, Y, X] (prediction.py:279-292)."""
    return vol.swapaxes(-1, -3)


def zyx2xyz(vol: np.ndarray) -> np.ndarray:
    """[..., Z, Y, X] -> [..., X, Y, Z] (prediction.py:295-307)."""
    return vol.swapaxes(-1, -3)


# storage types whose range guard can fire -> the plan of the same precision class with fp32's exponent range
_FALLBACK = {'f16': 'bf16', 'f16x2': 'f32'}
_ACT_NAMES = {'fp16': 'f16', 'float16': 'f16', 'bfloat16': 'bf16', 'fp32': 'f32', 'float32': 'f32', 'split': 'f16x2'}


# ------------------------------------------------------------------------------------------------------
class Predictor:
    """MI355X implementation of ``elektronn3.inference.Predictor`` (third-party; constructed at
    prediction.py:777-779 and :1062): tiled, overlap-and-crop inference of a 3D U-Net.

    Supported (= what SyConn's dense path uses): `model` as ``nn.Module`` or path to a TorchScript ``.pts`` /
    pickled ``.pt`` file, `state_dict_src`, `device`, `tile_shape`/`overlap_shape` (z,y,x), `out_shape`
    (C,z,y,x), `strict_shapes`, `apply_softmax`, `apply_argmax`, `float16`, `batch_size`, `verbose`.
    `transform`, `augmentations`, `offset` (valid convolutions) and `argmax_with_threshold` are unused by SyConn
    and rejected.

    Precision.  The reference computes in fp32 (`float16=False`, prediction.py:777-779).  `float16=False` (the default, what
    SyConn passes) therefore selects the REFERENCE-PRECISION plan 'f16x2': every activation and weight is kept as two fp16
    numbers hi + lo and every product is three matrix-core passes with fp32 accumulation -- logits within ~1e-6 of the fp32
    oracle's range (stated tolerance 1e-5), argmax / threshold-rule labels equal except where the oracle itself sits on a
    decision boundary, at ~3.4x the time of 'f16'.  `float16=True` (elektronn3: ``model.half()``) selects 'f16'.  The extra
    keyword `act_dtype` overrides both: 'f16x2', 'f16' (0.06 % of the threshold-rule labels of the 128^3 headline tile differ
    from the fp32 oracle, max logit error 8.7e-4 of the logit range), 'bf16' (0.45 %, 7.4e-3; fp32's exponent range, ~3 %
    faster than 'f16'; tests/test_gpu_labels_headline.py), or 'f32' (fp32 storage and FMA arithmetic
    off the matrix cores, ~30x slower than 'f16').  Accumulation is fp32 in every plan.  The fp16-based plans are
    range-guarded: an overflow (> 65504) is detected on the device; with `overflow_fallback` (default: on unless `act_dtype`
    was given explicitly) the prediction is repeated in the next plan with fp32's exponent range ('f16' -> 'bf16', 'f16x2' ->
    'f32') and the Predictor stays there, otherwise ``ActivationOverflowError`` (a ``RuntimeError``) is raised.
    `batch_size`: tiles per launch set (default: automatic,
    see `_batch_for`).  `n_streams` (default: 1, or 2 for single-tile launch sets; env SYCONN_AMD_STREAMS): batches alternate over that many HIP
    streams, each with its own workspace.

    ``predict(inp)`` takes an ``np.ndarray`` / ``Tensor`` of shape (N,1,D,H,W) and any float dtype and returns a
    float32 CPU tensor (N,C,D,H,W).  Device-memory exhaustion raises ``RuntimeError`` (the reference's
    tile-halving loop relies on that, prediction.py:783-794); `strict_shapes` violations raise ``ValueError``.
    """

    def __init__(self, model, state_dict_src=None, device=None, batch_size=None, tile_shape=None,
                 overlap_shape=None, offset=None, out_shape=None, out_dtype=None, float16=False,
                 apply_softmax=True, transform=None, augmentations=None, strict_shapes=False, apply_argmax=False,
                 argmax_with_threshold=None, verbose=False, report_inf_speed=False, act_dtype=None,
                 group_norm_groups=None, n_streams=None, defer_guard=False, overflow_fallback=None, clip_tiles=True,
                 sticky_fallback=True):
        from ..engine import DenseModel, StreamRing
        if transform is not None or augmentations is not None or argmax_with_threshold is not None:
            raise NotImplementedError('transform / augmentations / argmax_with_threshold are not used by SyConn\'s '
                                      'dense path and not implemented')
        if offset is not None and np.any(np.asarray(offset) != 0):
            raise NotImplementedError('valid-convolution offsets are not used by SyConn\'s dense path')
        if isinstance(model, str):
            model = os.path.expanduser(model)
            if not os.path.isfile(model):
                raise ValueError(f'Model path {model} not found.')
            if model.endswith('.pts'):
                model = torch.jit.load(model, map_location='cpu')
            elif model.endswith('.pt'):
                model = torch.load(model, map_location='cpu', weights_only=False)
            else:
                raise ValueError(f'{model} has an unknown file extension. Supported are: .pt and .pts')
        if isinstance(state_dict_src, str):
            state_dict_src = torch.load(state_dict_src, map_location='cpu', weights_only=False)
            state_dict_src = state_dict_src.get('model_state_dict', state_dict_src)
        if state_dict_src is not None and not isinstance(model, dict):
            model.load_state_dict(state_dict_src)
        if hasattr(model, 'eval'):
            model.eval()
        self.model = model
        if device is None:
            device = torch.device('cuda', torch.cuda.current_device()) if torch.cuda.is_available() else None
        if device is None or torch.device(device).type != 'cuda':
            raise RuntimeError('syconn_amd.Predictor needs an MI355X (ROCm device); there is no CPU fallback')
        self.device = torch.device(device)
        self.batch_size = batch_size
        self.tile_shape = None if tile_shape is None else np.asarray(tile_shape, dtype=np.int64)
        self.overlap_shape = None if overlap_shape is None else np.asarray(overlap_shape, dtype=np.int64)
        if self.overlap_shape is not None and np.any(self.overlap_shape < 0):
            raise ValueError('overlap_shape must be non-negative')
        self.out_shape = None if out_shape is None else tuple(int(s) for s in out_shape)
        self.out_dtype = torch.float32 if out_dtype is None else out_dtype
        self.float16 = float16
        self.apply_softmax = apply_softmax
        self.strict_shapes = strict_shapes
        self.apply_argmax = apply_argmax
        self.verbose = verbose
        self.report_inf_speed = report_inf_speed
        # fp16 range guard: fp16 storage overflows above 65504 (the reference computes in fp32 and cannot).  The library flags
        # it (sd_model_overflow).  With `overflow_fallback` the prediction is then repeated in the plan of the same precision
        # class that has fp32's exponent range (_FALLBACK) and the Predictor stays there; without it ActivationOverflowError is
        # raised.  Default: on for the default storage type, off for an explicitly requested one.
        self._fallback = (act_dtype is None) if overflow_fallback is None else bool(overflow_fallback)
        # `sticky_fallback`: after an overflow the Predictor STAYS in the fallback plan (default; 'f16x2' -> 'f32' is ~9x slower).  False:
        # only the prediction that overflowed is repeated there and the next one runs in the configured plan again (what dense_predictor
        # asks for: one hot chunk must not slow the worker's remaining chunks); `n_fallbacks` counts the repeats either way.
        self.sticky_fallback = bool(sticky_fallback)
        self.n_fallbacks = 0
        self._dm_fallback = None
        # `defer_guard`: do not synchronise after every prediction (pipelined callers); the caller asks `overflowed()` once
        # its stream of predictions is done and repeats them in bf16 itself
        self.defer_guard = bool(defer_guard)
        # tiles that overhang the volume are predicted on the part of their window that matters (see `_tiled`); same values
        self.clip_tiles = bool(clip_tiles)
        if act_dtype is None:
            # the reference's precision is what `float16` says: False (SyConn's call, prediction.py:777-779) = fp32 results ->
            # the split-fp16 reference-precision plan; True (elektronn3: model.half()) = fp16 storage
            act_dtype = 'f16' if float16 else 'f16x2'
        act_dtype = _ACT_NAMES.get(act_dtype, act_dtype)
        self.act_dtype = act_dtype
        self._gn_groups = group_norm_groups
        self._dm = DenseModel(model, act_dtype=act_dtype, device=self.device, group_norm_groups=group_norm_groups)
        self.out_channels = self._dm.out_channels
        # HIP streams that tiles alternate over.  Given (argument or SYCONN_AMD_STREAMS): that many, always.  Default: one, and
        # two for tiles that run one per launch set (the reference's 178 x 243 x 331 windows): the small deep layers and the
        # launch tail of one tile then run under the big layers of the next (+2.5 ... 5 % on the reference geometry; batches of
        # 128^3 tiles fill the GPU by themselves: +-0)
        if n_streams is None and 'SYCONN_AMD_STREAMS' in os.environ:
            n_streams = int(os.environ['SYCONN_AMD_STREAMS'])
        self._ring = StreamRing(self.device, 1 if n_streams is None else n_streams)
        self._ring2 = StreamRing(self.device, 2) if n_streams is None else None

    # -- geometry --------------------------------------------------------------------------------------
    def _geometry(self, spatial: np.ndarray):
        tile = spatial.copy() if self.tile_shape is None else self.tile_shape
        ol = np.zeros(3, dtype=np.int64) if self.overlap_shape is None else self.overlap_shape
        if len(tile) != 3 or len(ol) != 3:
            raise ValueError('tile_shape / overlap_shape must have 3 entries (z, y, x)')
        if self.out_shape is not None:
            if self.out_shape[0] != self.out_channels:
                raise ValueError(f'out_shape[0]={self.out_shape[0]} but the model predicts {self.out_channels} '
                                 f'channels')
            if tuple(self.out_shape[1:]) != tuple(int(s) for s in spatial):
                raise ValueError(f'out_shape {self.out_shape} does not match the input shape {tuple(spatial)}')
        if np.any(spatial % tile != 0):
            if self.strict_shapes:
                raise ValueError(f'spatial inp shape {tuple(spatial)} has to be divisible by '
                                 f'tile_shape {tuple(tile)} (strict_shapes=True)')
            if np.any(tile > spatial):
                tile = np.minimum(tile, spatial)
        ntiles = np.ceil(spatial / tile).astype(np.int64)
        return tile, ol, ntiles

    def _tiled(self, vol: torch.Tensor, out: torch.Tensor, out_kind: int, label_args=None, halo_included: bool = False,
               valid_box=None):
        """tiled_apply (elektronn3) on the device: zero-padded tile extraction, forward,
        crop of the overlap, write into `out` (C,D,H,W).  vol: (D,H,W) uint8 / float32 on the device.
        `halo_included`: `vol` already carries `overlap_shape` voxels of REAL neighbouring data per side (zeros where the
        dataset ends) instead of being zero-padded here; `out` then covers the inner region only.  This is how a chunk of a
        larger volume is predicted so that the result equals the same tile grid run over the whole volume.
        `valid_box` = ((z0, y0, x0), (z1, y1, x1)) in `out` coordinates: the part of `out` that lies INSIDE the dataset.  The
        reference's chunk grid (``fit_box_size=True``, prediction.py:679-683) covers up to 1.9x the dataset and it predicts
        every tile of every chunk, also those whose whole (cropped) result lies beyond the dataset boundary -- values of a
        zero input that nothing downstream reads.  With a `valid_box` such tiles are not predicted (their region of `out` is
        zero); every voxel inside the dataset is unchanged, because a tile's result depends on nothing but that tile.
        `self.clip_tiles`: a tile that reaches beyond `vol` or the `valid_box` (the dataset ends inside it; or its outer rim
        is the chunk's halo ring, which dense_predictor crops at prediction.py:812) is predicted on the part of its window the
        wanted voxels can depend on (`sd_plan_clip_window`: the borders of every layer stay outside their cones) -- same
        values, less arithmetic; beyond the box `out` is zero; networks with GroupNorm (whole-tile statistics) keep full windows."""
        from ..engine import tile_gather, tile_scatter
        ol_in = np.zeros(3, dtype=np.int64) if self.overlap_shape is None else self.overlap_shape
        spatial = np.asarray(vol.shape, dtype=np.int64) - (2 * ol_in if halo_included else 0)
        shift = ol_in if halo_included else np.zeros(3, dtype=np.int64)
        tile, ol, ntiles = self._geometry(spatial)
        tin = tile + 2 * ol
        single = bool(np.all(ntiles == 1) and np.all(ol == 0) and np.all(tile == spatial) and not halo_included)
        nch = 1 if label_args is not None else self.out_channels

        def run(inp, outp, slot, roi=None):           # inp (n,D,H,W) -> outp (n,nch,D,H,W); roi: the part of the window that is kept
            if label_args is not None:
                self._dm.forward_labels_batch(inp, label_args[0], label_args[1], out=outp[:, 0], slot=slot, roi=roi)
            else:
                self._dm.forward_batch(inp, out_kind, outp, slot=slot, roi=roi)

        if single:
            run(vol[None], out[None], 0)
            return
        # independent tiles go through the network `nb` at a time (sd_forward_batch: one set of launches, every
        # kernel sees nb times as many blocks); batches alternate over `n_streams` HIP streams.
        # Which tiles run, on which window (full, or clipped at the far side to what the wanted voxels depend on), keeping which box:
        # syconn_amd.tiling.plan_tile_windows -- the same arithmetic parallel.predict_volume_distributed orders its rounds by
        from ..tiling import plan_tile_windows
        by_window, zero = plan_tile_windows(spatial, tile, ol, ntiles, valid_box, self.clip_tiles, self._dm.clipped_window,
                                            self._dm.has_groupnorm)
        if not by_window:
            out.zero_()
            return
        if zero:                                 # beyond the dataset `out` reads zero, whatever was skipped or clipped
            out.zero_()
        nb = self._batch_for(tin, max(len(g) for g in by_window.values()))
        n_tiles = sum(len(g) for g in by_window.values())
        ring = self._ring2 if (self._ring2 is not None and nb == 1 and n_tiles > 1) else self._ring
        tbuf = [torch.empty(nb * int(np.prod(tin)), dtype=vol.dtype, device=self.device) for _ in range(ring.n)]
        obuf = [torch.empty(nb * nch * int(np.prod(tin)), dtype=out.dtype, device=self.device) for _ in range(ring.n)]
        i = 0
        with ring:
            for (win, roi), tiles in by_window.items():
                nvox = int(np.prod(win))
                for b0 in range(0, len(tiles), nb):
                    group = tiles[b0:b0 + nb]
                    n, k = len(group), ring.slot(i)
                    tb = tbuf[k][:n * nvox].view(n, *win)
                    ob = obuf[k][:n * nch * nvox].view(n, nch, *win)
                    with ring.stream(i):
                        for j, (lo, start, _, _) in enumerate(group):
                            tile_gather(vol, lo - ol + shift + start, win, tb[j])
                        run(tb, ob, k, roi)
                        for j, (lo, start, w0, w1) in enumerate(group):
                            tile_scatter(ob[j], ol + w0 - start, w1 - w0, out, lo + w0)
                    i += 1

    def chunk_cost_model(self, halo, halo_included: bool, skip_outside: bool = True):
        """Cost of a chunk of a chunked volume prediction through this Predictor, from geometry alone (``syconn_amd.tiling``)."""
        from ..tiling import ChunkCostModel, PlanClipper
        return ChunkCostModel(PlanClipper(self._dm._ops_arr), self.tile_shape, self.overlap_shape, halo, halo_included,
                              self.clip_tiles, skip_outside)

    def _guarded(self, run):
        """Run one tiled prediction; if the fp16 range guard fired, repeat it in bf16 (default storage type) or raise."""
        from ..engine import DenseModel
        run()
        if self.defer_guard or self.act_dtype not in _FALLBACK or not self._dm.overflowed():
            return
        nxt = _FALLBACK[self.act_dtype]
        if not self._fallback:
            raise L.ActivationOverflowError(
                f"fp16 activation overflow (a stored activation exceeded 65504): results invalid; use act_dtype='{nxt}'")
        self.n_fallbacks += 1
        if self._dm_fallback is None:
            self._dm_fallback = DenseModel(self.model, act_dtype=nxt, device=self.device, group_norm_groups=self._gn_groups)
        if self.sticky_fallback:
            log_main.warning(f'syconn_amd.Predictor: fp16 activation overflow detected -- switching this Predictor from '
                             f'{self.act_dtype} to {nxt} storage and repeating the prediction')
            self.act_dtype = nxt
            self._dm, self._dm_fallback = self._dm_fallback, None
            run()
            return
        log_main.warning(f'syconn_amd.Predictor: fp16 activation overflow detected -- repeating this prediction in {nxt} storage '
                         f'(fallback {self.n_fallbacks}); the next one runs in {self.act_dtype} again')
        main, self._dm = self._dm, self._dm_fallback
        try:
            run()
        finally:
            self._dm = main

    def overflowed(self) -> bool:
        """fp16 range guard of the predictions since the last call (synchronises the current stream); for `defer_guard`."""
        return self._dm.overflowed()

    @torch.no_grad()
    def probe_memory(self, spatial_shape) -> None:
        """What dense_predictor's warm-up prediction of a zero chunk is for (prediction.py:781-794: a CUDA out-of-memory
        ``RuntimeError`` there makes the caller halve the tile shape): reserve everything a prediction of a (D,H,W) volume holds
        at the same time -- result tensor, tile and output buffers and the workspaces of every stream for the largest window --
        and run ONE launch set of zero tiles per stream (first-launch costs of the kernels), instead of predicting all tiles of
        the chunk (12 in the reference's geometry: 0.2 s of a worker's life in the reference-precision plan)."""
        spatial = np.asarray(spatial_shape, dtype=np.int64)
        tile, ol, ntiles = self._geometry(spatial)
        tin = tile + 2 * ol
        n_all = int(np.prod(ntiles))
        nb = self._batch_for(tin, n_all)
        ring = self._ring2 if (self._ring2 is not None and nb == 1 and n_all > 1) else self._ring
        torch.cuda.set_device(self.device)
        shape = [int(t) for t in tin]
        out = torch.empty((self.out_channels, *[int(s) for s in spatial]), dtype=torch.uint8, device=self.device)
        tb = [torch.zeros((nb, *shape), dtype=torch.uint8, device=self.device) for _ in range(ring.n)]
        ob = [torch.empty((nb, self.out_channels, *shape), dtype=torch.uint8, device=self.device) for _ in range(ring.n)]
        roi = (tuple(int(v) for v in ol), tuple(int(v) for v in ol + tile)) if (self.clip_tiles and np.any(ol > 0)) else None
        # (a tile with another box -- boundary tiles keep whole windows, the level-0 decoder is replaced by its layers -- may need a
        # larger workspace than the interior one: reserve for both forms, inside the caller's tile-halving try block)
        with ring:
            for r in ([roi, None] if roi is not None else [None]):
                for k in range(ring.n):
                    with ring.stream(k):
                        self._dm.forward_batch(tb[k], L.SD_OUT_PROBS_U8, ob[k], slot=ring.slot(k), roi=r)
        torch.cuda.current_stream(self.device).synchronize()
        self._dm.overflowed()                    # (clears the range-guard flag; zeros cannot overflow)
        del out, tb, ob

    def _batch_for(self, tin, ntiles: int) -> int:
        """Tiles per launch set: `batch_size` if given (elektronn3's Predictor argument), else as many as keep the
        workspaces of one batch under ~8 GiB (at most 8): 128^3 tiles run 8 at a time, the reference's
        178x243x331 tiles (7.4 GiB of activations each) one at a time."""
        if self.batch_size is not None:
            return max(1, min(int(self.batch_size), ntiles))
        per_tile = self._dm.workspace_bytes(tuple(int(t) for t in tin))
        return int(max(1, min(8, ntiles, (8 << 30) // max(per_tile, 1))))

    # -- public API ------------------------------------------------------------------------------------
    @torch.no_grad()
    def predict(self, inp: Union[np.ndarray, torch.Tensor]) -> torch.Tensor:
        """(N,1,D,H,W) float -> (N,C,D,H,W) float32 CPU tensor (rows P2/P4; called at prediction.py:781, 863)."""
        if isinstance(inp, np.ndarray):
            inp = torch.from_numpy(np.ascontiguousarray(inp))
        if inp.dim() != 5:
            raise ValueError(f'expected (N, C, D, H, W) input, got shape {tuple(inp.shape)}')
        if inp.shape[1] != 1:
            raise ValueError('the dense path feeds single-channel EM data (C must be 1)')
        n = inp.shape[0]
        spatial = tuple(int(s) for s in inp.shape[2:])
        out = torch.empty((n, self.out_channels, *spatial), dtype=torch.float32)
        kind = L.SD_OUT_PROBS_F32 if self.apply_softmax else L.SD_OUT_LOGITS_F32
        torch.cuda.set_device(self.device)
        out_dev = torch.empty((self.out_channels, *spatial), dtype=torch.float32, device=self.device)
        for b in range(n):
            vol = inp[b, 0].to(torch.float32).contiguous().to(self.device)
            self._guarded(lambda: self._tiled(vol, out_dev, kind))
            out[b] = out_dev.cpu()
        if self.apply_argmax:
            out = out.argmax(1)
        return out

    @torch.no_grad()
    def predict_proba_u8_device(self, raw_u8: torch.Tensor, halo_included: bool = False, valid_box=None) -> torch.Tensor:
        """Fast path of ``dense_predicton_helper(raw.astype(float32)/255., self)``: `raw_u8` is the (D,H,W) uint8
        chunk ON THE DEVICE; returns uint8 ``floor(255*softmax)`` (C,D,H,W) on the device.  Bit-identical to the
        slow path by construction: the kernel normalises with the table float32(v)/255 (prediction.py:808) and
        truncates the float32 product p*255 (prediction.py:864-865)."""
        if not self.apply_softmax:
            raise ValueError('uint8 probabilities need apply_softmax=True')
        assert raw_u8.dtype == torch.uint8 and raw_u8.dim() == 3
        torch.cuda.set_device(self.device)
        raw_u8 = raw_u8.contiguous()
        inner = tuple(int(s) - (2 * int(o) if halo_included else 0) for s, o in
                      zip(raw_u8.shape, (self.overlap_shape if self.overlap_shape is not None else (0, 0, 0))))
        out = torch.empty((self.out_channels, *inner), dtype=torch.uint8, device=self.device)
        self._guarded(lambda: self._tiled(raw_u8, out, L.SD_OUT_PROBS_U8, halo_included=halo_included, valid_box=valid_box))
        return out


    @torch.no_grad()
    def predict_labels_u8_device(self, raw_u8: torch.Tensor, ids, thresholds, halo_included: bool = False,
                                 valid_box=None) -> torch.Tensor:
        """`predict_proba_u8_device` followed by the label rule of dense_predictor (prediction.py:813-833) for ONE
        multi-id target, evaluated in the network's final epilogue: (D,H,W) uint8 labels on the device.  `thresholds`
        are the resolved uint8-scale values, one per id."""
        if not self.apply_softmax:
            raise ValueError('labels need apply_softmax=True')
        assert raw_u8.dtype == torch.uint8 and raw_u8.dim() == 3
        torch.cuda.set_device(self.device)
        raw_u8 = raw_u8.contiguous()
        inner = tuple(int(s) - (2 * int(o) if halo_included else 0) for s, o in
                      zip(raw_u8.shape, (self.overlap_shape if self.overlap_shape is not None else (0, 0, 0))))
        out = torch.empty((1, *inner), dtype=torch.uint8, device=self.device)
        self._guarded(lambda: self._tiled(raw_u8, out, L.SD_OUT_PROBS_U8,
                                          label_args=([int(i) for i in ids], [float(t) for t in thresholds]),
                                          halo_included=halo_included, valid_box=valid_box))
        return out[0]


# ------------------------------------------------------------------------------------------------------
def dense_predicton_helper(raw: np.ndarray, predictor: 'Predictor', is_zyx=False, return_zyx=False) -> np.ndarray:
    """prediction.py:846-868.  `raw`: float array (X,Y,Z) or (Z,Y,X) already scaled to 0..1; returns the
    inference result as uint8 (C, ...) between 0..255 (truncated ``pred*255``)."""
    vol_zyx = raw if is_zyx else xyz2zyx(raw)
    probs = predictor.predict(vol_zyx[None, None]).numpy()[0]           # (C, Z, Y, X) float32, batch axis dropped
    out = (np.array(probs) * 255).astype(np.uint8)                      # float32 product, truncating cast (:864-865)
    return out if return_zyx else zyx2xyz(out)


def _resolve_threshold(t) -> float:
    """prediction.py:824-827: ``None -> 255/2``; ``t < 1 -> 255*t``."""
    if t is None:
        t = 255 / 2
    if t < 1.:
        t = 255 * t
    return float(t)


def dense_predictor(args):
    """Worker of the dense prediction (one process = one GPU), prediction.py:723-843.  `args` is the reference's
    14-tuple ``(chunk_ids, kd_p, target_p, model_p, overlap_shape, overlap_shape_tiles, tile_shape, chunk_size,
    n_channel, target_channels, target_kd_path_list, channel_thresholds, mag, cube_of_interest)``.

    Differences to the reference are confined to WHERE the arithmetic runs: the uint8 chunk goes to the GPU once,
    normalisation, tiling, U-Net, softmax, uint8 cast, halo crop and the label rule run there, and only uint8
    results come back (the reference moves fp32 tiles over PCIe in both directions)."""
    from ..engine import mag_pyramid, postproc_labels, tile_scatter
    chunk_ids, kd_p, target_p, model_p, overlap_shape, overlap_shape_tiles, tile_shape, chunk_size, n_channel, \
        target_channels, target_kd_path_list, channel_thresholds, mag, cube_of_interest = args
    import time as _time
    t_start = _time.perf_counter()

    kd = KnossosDataset()
    kd.initialize_from_knossos_path(kd_p)
    cd = ChunkDataset()
    cd.initialize(kd, cube_of_interest[1], chunk_size, target_p + '/cd_tmp/', box_coords=cube_of_interest[0],
                  list_of_coords=[], fit_box_size=True, overlap=overlap_shape)
    target_kd_dict = {path: basics.kd_factory(path) for path in target_kd_path_list}
    if not os.environ.get('SYCONN_AMD_NO_WRITE_COMBINING'):
        # chunks are not aligned to the target cubes: assemble the cubes this worker touches in memory and write each once
        # (KnossosDataset.enable_write_combining; flushed at the end of this worker)
        for tkd in target_kd_dict.values():
            tkd.enable_write_combining(chunk_shape=chunk_size)

    ix = 0
    tile_shape = np.array(tile_shape)
    overlap_shape = np.asarray(overlap_shape)
    overlap_shape_tiles = np.asarray(overlap_shape_tiles)
    chunk_size = np.asarray(chunk_size)
    # storage type of the activations: config['dense_prediction']['act_dtype']; default 'f16x2' = the reference's precision
    # (the fast plans 'f16' / 'bf16' are an explicit configuration choice).  A range-guard overflow on any chunk falls back
    # to the plan with fp32's exponent range instead of killing the worker.
    act_dtype = global_params.config['dense_prediction']['act_dtype'] if _wd_set() else 'f16x2'
    skip_outside = bool(global_params.config['dense_prediction'].get('skip_tiles_outside_dataset', True)) if _wd_set() else True
    clip_tiles = bool(global_params.config['dense_prediction'].get('clip_boundary_tiles', True)) if _wd_set() else True
    sticky = bool(global_params.config['dense_prediction'].get('sticky_overflow_fallback', False)) if _wd_set() else False
    log_main.info(f'dense_predictor: activation storage type {act_dtype} '
                  f'({"reference precision" if act_dtype in ("f16x2", "f32") else "reduced precision, fast plan"})')
    while True:
        try:
            out_shape = (chunk_size + 2 * np.array(overlap_shape)).astype(np.int32)[::-1]  # ZYX
            out_shape = np.insert(out_shape, 0, n_channel)  # output must equal chunk size
            predictor = Predictor(model_p, strict_shapes=True, tile_shape=tile_shape[::-1], out_shape=out_shape,
                                  overlap_shape=overlap_shape_tiles[::-1], apply_softmax=True, act_dtype=act_dtype,
                                  overflow_fallback=True, clip_tiles=clip_tiles, sticky_fallback=sticky)
            try:
                predictor.model.ae = False
            except Exception:  # ScriptModules refuse new attributes; elektronn3's flag has no meaning here
                pass
            # warm-up / memory probe for a full-size chunk (prediction.py:781 predicts float64 zeros of that size)
            if os.environ.get('SYCONN_AMD_FULL_WARMUP'):      # (A/B switch: the reference's full-chunk warm-up)
                _ = predictor.predict_proba_u8_device(
                    torch.zeros(tuple(int(s) for s in out_shape[1:]), dtype=torch.uint8, device=predictor.device))
            else:
                predictor.probe_memory(tuple(int(s) for s in out_shape[1:]))
            break
        except L.ActivationOverflowError:      # (a RuntimeError, but not a memory problem: halving tiles would not help)
            raise
        except RuntimeError:  # device MemoryError
            if np.all(tile_shape % 2):
                raise ValueError('Cannot reduce tile shape anymore. Please adapt the tile/overlap/chunk shape in '
                                 'the function that is calling `dense_predictor`.')
            while tile_shape[ix] % 2:
                ix += 1
            tile_sh_orig = np.array(tile_shape)
            tile_shape[ix] = tile_shape[ix] // 2
            log_main.warning(f'Changed tile shape from {tile_sh_orig} to {tile_shape} to reduce memory requirements.')
            ix = (ix + 1) % 3

    # Host I/O is pipelined around the GPU: one thread reads chunk k+1 from the KnossosDataset while chunk k is
    # predicted, one thread writes the results of chunk k-1 (cube files of neighbouring chunks overlap, so writes stay
    # sequential and in chunk order).  The reference does read -> predict -> write strictly in sequence.
    from concurrent.futures import ThreadPoolExecutor
    dev = predictor.device
    torch.cuda.set_device(dev)
    s_in, s_out = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)

    spent = {'read': 0.0, 'gpu': 0.0, 'write': 0.0}       # seconds per pipeline stage (SYCONN_AMD_IO_TIMING=1 logs them)
    t_setup = _time.perf_counter() - t_start              # datasets opened, model planned, workspace reserved

    read_bufs = {}

    def read_chunk(ch_id):
        t0 = _time.perf_counter()
        ch = cd.chunk_dict[ch_id]
        ol = ch.overlap
        size = np.array(np.array(ch.size) + 2 * np.array(ol), dtype=np.int32)
        coords = np.array(np.array(ch.coordinates) - np.array(ol), dtype=np.int32)
        # page-locked read buffers, reused round robin (3: one being filled, one uploading, one spare): a fresh 80 MB array per
        # chunk costs its page faults, and a pageable upload runs at a fraction of the link rate
        shape_zyx = tuple(int(s) for s in size[::-1])
        if read_bufs.get('shape') != shape_zyx:
            read_bufs.update(shape=shape_zyx, bufs=[torch.empty(shape_zyx, dtype=torch.uint8).pin_memory() for _ in range(3)], evs=[None] * 3, k=0)
        k = read_bufs['k'] % 3
        read_bufs['k'] += 1
        if read_bufs['evs'][k] is not None:
            read_bufs['evs'][k].synchronize()            # its previous upload has left the buffer
        hbuf = read_bufs['bufs'][k]
        if isinstance(kd, KnossosDataset):
            kd.load_raw(size=size * mag, offset=coords * mag, mag=mag, out=hbuf.numpy())          # uint8, ZYX
        else:                                            # (a foreign dataset object: its own allocation, then one copy)
            hbuf.numpy()[...] = kd.load_raw(size=size * mag, offset=coords * mag, mag=mag)
        with torch.cuda.stream(s_in):
            out_dev = hbuf.to(dev, non_blocking=True)
            ev = s_in.record_event()
        read_bufs['evs'][k] = ev
        spent['read'] += _time.perf_counter() - t0
        return out_dev, ev

    pin_pool = {}                        # page-locked download buffers by shape (a pageable D2H copy runs at a fraction of the link rate)

    def write_chunk(jobs, ev):
        t0 = _time.perf_counter()
        # download on the copy-out stream, from the writer thread: only waits for THIS chunk's kernels (event), not for the
        # next chunk's work that the main thread has queued on the compute stream meanwhile
        host = []
        with torch.cuda.stream(s_out):
            s_out.wait_event(ev)
            for save, kwargs, lvl in jobs:
                free = pin_pool.setdefault(tuple(lvl.shape), [])
                h = free.pop() if free else torch.empty(tuple(lvl.shape), dtype=lvl.dtype).pin_memory()
                h.copy_(lvl, non_blocking=True)
                host.append((save, kwargs, h))
            s_out.synchronize()
        for save, kwargs, h in host:
            save(data=h.numpy(), **kwargs)       # (uint8 labels of an overlay dataset are widened cube by cube inside save_seg)
            pin_pool[tuple(h.shape)].append(h)
        spent['write'] += _time.perf_counter() - t0

    class _Inline:                       # SYCONN_AMD_SEQ_IO=1: no overlap, everything in the caller's thread (debugging / A-B)
        def __enter__(self):
            return self

        def __exit__(self, *exc):
            return False

        def submit(self, fn, *a):
            from concurrent.futures import Future
            f = Future()
            f.set_result(fn(*a))
            return f

    seq_io = bool(os.environ.get('SYCONN_AMD_SEQ_IO'))
    chunk_ids = list(chunk_ids)
    with (_Inline() if seq_io else ThreadPoolExecutor(max_workers=1)) as reader, \
            (_Inline() if seq_io else ThreadPoolExecutor(max_workers=1)) as writer:
        nxt = reader.submit(read_chunk, chunk_ids[0]) if chunk_ids else None
        writes = []
        for n, ch_id in enumerate(chunk_ids):
            ch = cd.chunk_dict[ch_id]
            ol = ch.overlap
            raw_dev, ev_in = nxt.result()
            nxt = reader.submit(read_chunk, chunk_ids[n + 1]) if n + 1 < len(chunk_ids) else None
            t_gpu = _time.perf_counter()
            cur = torch.cuda.current_stream(dev)
            cur.wait_event(ev_in)
            raw_dev.record_stream(cur)
            # one multi-id target (mivcsj, syntype): only its label volume is needed -> label rule in the final epilogue
            only_labels = len(target_channels) == 1 and len(target_channels[0]) > 1
            # the chunk grid (fit_box_size=True) overhangs the dataset: model tiles whose whole cropped result lies beyond the
            # boundary (or in the halo ring that is cropped below) are not predicted -- zeros instead of the network's answer to
            # a zero input, in a region nothing reads (config['dense_prediction']['skip_tiles_outside_dataset'])
            vbox = None
            if skip_outside:
                c0 = np.asarray(ch.coordinates) - np.asarray(ol)                      # origin of chunk + halo, xyz
                v_lo = np.maximum(np.asarray(ol), -c0)
                v_hi = np.minimum(np.asarray(ol) + np.asarray(ch.size), np.asarray(kd.boundary) // mag - c0)
                vbox = (tuple(int(v) for v in v_lo[::-1]), tuple(int(v) for v in v_hi[::-1]))
            if only_labels:
                ids0 = target_channels[0]
                thr0 = [_resolve_threshold(channel_thresholds[label]) for label in ids0]
                pred_dev = predictor.predict_labels_u8_device(raw_dev, ids0, thr0, valid_box=vbox)[None]   # (1, Z, Y, X) uint8 labels
            else:
                pred_dev = predictor.predict_proba_u8_device(raw_dev, valid_box=vbox)   # (C, Z, Y, X) uint8
            # slice out the original input volume along ZYX (prediction.py:812)
            zyx = tuple(int(s) for s in np.asarray(ch.size)[::-1])
            crop = torch.empty((pred_dev.shape[0], *zyx), dtype=torch.uint8, device=dev)
            tile_scatter(pred_dev, (int(ol[2]), int(ol[1]), int(ol[0])), zyx, crop, (0, 0, 0))
            jobs = []
            for j in range(len(target_channels)):
                ids = target_channels[j]
                path = target_kd_path_list[j]
                save_as_raw = not (len(ids) > 1)
                # the mag pyramid [mag, 2*mag, 4*mag] (order-0, fast_resampling=True) is built on the device; each level
                # is written with its own data_mag, which is what one save_*(mags=[mag, 2*mag, 4*mag]) call produces
                if save_as_raw:
                    # no thresholding and only one label in the target KnossosDataset -> store probability map
                    for k, lvl in enumerate(mag_pyramid(crop[ids[-1]], 3)):
                        lvl.record_stream(s_out)
                        jobs.append((target_kd_dict[path].save_raw,
                                     dict(offset=ch.coordinates * mag, data_mag=mag * 2 ** k,
                                          mags=[mag * 2 ** k], fast_resampling=True, upsample=False), lvl))
                else:
                    thr = [_resolve_threshold(channel_thresholds[label]) for label in ids]
                    lab = crop[0] if only_labels else postproc_labels(crop, ids, thr, out_dtype=torch.uint8)
                    for k, lvl in enumerate(mag_pyramid(lab, 3)):  # uint8 on the device and over PCIe, widened by the writer
                        lvl.record_stream(s_out)
                        jobs.append((target_kd_dict[path].save_seg,
                                     dict(offset=ch.coordinates * mag, data_mag=mag * 2 ** k, mags=[mag * 2 ** k],
                                          fast_resampling=True, upsample=False), lvl))
            ev_done = cur.record_event()
            spent['gpu'] += _time.perf_counter() - t_gpu
            writes.append(writer.submit(write_chunk, jobs, ev_done))
            while len(writes) > 2:                   # bound the host memory held by queued results
                writes.pop(0).result()
        for w in writes:
            w.result()
    t0 = _time.perf_counter()
    for tkd in target_kd_dict.values():
        tkd.flush()
    t_flush = _time.perf_counter() - t0
    spent['write'] += t_flush
    if predictor.n_fallbacks:
        log_main.warning(f'dense_predictor: {predictor.n_fallbacks} of {len(chunk_ids)} chunk(s) overflowed fp16 storage and were predicted '
                         f'in the fallback plan ({_FALLBACK.get(act_dtype, "?")})')
    if os.environ.get('SYCONN_AMD_IO_TIMING'):
        log_main.warning('dense_predictor stages over %d chunk(s): read + H2D %.2f s (reader thread), launch %.2f s (main thread), '
                         'D2H + write %.2f s (writer thread; includes waiting for the kernels and %.2f s of final flush); setup %.2f s, total %.2f s',
                         len(chunk_ids), spent['read'], spent['gpu'], spent['write'], t_flush, t_setup, _time.perf_counter() - t_start)


def _wd_set() -> bool:
    try:
        _ = global_params.config.working_dir
        return True
    except ValueError:
        return False


def _dense_targets(n_channel, target_names, target_channels, channel_thresholds):
    """Defaults and validation of the per-target arguments (prediction.py:655-664): one target 'pred' holding every
    channel, no thresholds; names and channel tuples must pair up."""
    names = ['pred'] if target_names is None else list(target_names)
    channels = [list(range(n_channel))] if target_channels is None else [list(c) for c in target_channels]
    if len(names) != len(channels):
        msg = 'For every target name the target channels have to be specified.'
        log_reps.error(msg)
        raise ValueError(msg)
    thresholds = [None] * n_channel if channel_thresholds is None else list(channel_thresholds)
    return names, channels, thresholds


def _dense_geometry():
    """(overlap, tile overlap, chunk size, tile shape) in x,y,z.  The reference hard-codes them and marks them as
    future config parameters (prediction.py:671-677); here they are ``config['dense_prediction']`` with those values as
    defaults.  Chunk halo == tile halo, as in the reference."""
    geo = global_params.config['dense_prediction']
    halo = np.array(geo['overlap_shape_tiles'])
    return halo, halo, np.array(geo['chunk_size']), list(geo['tile_shape'])


def _create_target_kds(paths, kd, cube_shape_kd, overwrite, log):
    """One empty KnossosDataset per target with a 6-level mag list and a knossos.conf (prediction.py:685-706).
    All existence checks run before anything is deleted or created, so a refused call leaves every target untouched."""
    existing = [p for p in paths if os.path.isdir(p)]
    if existing and not overwrite:
        msg = f'Found existing KD at "{existing[0]}" but overwrite is set to False.'
        log.error(msg)
        raise ValueError(msg)
    for p in existing:
        log.debug('Found existing KD at {}. Removing it now.'.format(p))
        shutil.rmtree(p)
    scale = np.array(global_params.config['scaling'])
    mags = [1 << k for k in range(6)]
    for p in paths:
        tkd = KnossosDataset()
        tkd._cube_shape = cube_shape_kd
        tkd.scales = [scale, ]
        tkd.initialize_without_conf(p, kd.boundary, kd.scale, kd.experiment_name, mags, create_pyk_conf=False,
                                    create_knossos_conf=True)
        try:
            basics.kd_factory(p)
        except ValueError as e:
            log.error(f'Could not initialize KnossosDataset at "{p}". {e}')


def predict_dense_to_kd(kd_path: str, target_path: str, model_path: str, n_channel: int,
                        target_names: Optional[Iterable[str]] = None,
                        target_channels: Optional[Iterable[Iterable[int]]] = None,
                        channel_thresholds: Optional[Iterable[Union[float, Any]]] = None,
                        log: Optional[Logger] = None, mag: int = 1,
                        overlap_shape_tiles: Tuple[int, int, int] = (40, 40, 20),
                        cube_of_interest: Optional[Tuple[np.ndarray]] = None, overwrite: bool = False,
                        cube_shape_kd: Optional[Tuple[int]] = None):
    """Dense prediction of a whole KnossosDataset into target KnossosDataset(s), prediction.py:594-720: builds the
    chunk grid, creates the target datasets, partitions the chunk ids round-robin over ``config.ngpu_total`` workers
    (``chunkify``) and dispatches one worker per GPU.

    As in the reference the keyword `overlap_shape_tiles` is overridden by the configured geometry
    (prediction.py:671-677 hard-codes it; here it is ``config['dense_prediction']``, same defaults)."""
    from ..mp import batchjob_utils as qu
    conf = global_params.config
    if log is None:
        log = initialize_logging('dense_predictions', conf.working_dir + '/logs/', overwrite=False)
    names, channels, thresholds = _dense_targets(n_channel, target_names, target_channels, channel_thresholds)
    overlap_shape, overlap_shape_tiles, chunk_size, tile_shape = _dense_geometry()

    kd = basics.kd_factory(kd_path)
    coi = (np.zeros(3, ), kd.boundary // mag) if cube_of_interest is None else cube_of_interest
    grid = ChunkDataset()
    grid.initialize(kd, coi[1], chunk_size, target_path + '/cd_tmp/', box_coords=coi[0], list_of_coords=[],
                    fit_box_size=True, overlap=overlap_shape)
    chunk_ids = list(grid.chunk_dict.keys())

    target_kds = [f'{target_path}/{name}/' for name in names]
    _create_target_kds(target_kds, kd, (256, 256, 256) if cube_shape_kd is None else cube_shape_kd, overwrite, log)

    # one 14-tuple per worker: its share of the chunk ids (static round-robin) + everything needed to rebuild the state
    shared = (kd_path, target_path, model_path, overlap_shape, overlap_shape_tiles, tile_shape, chunk_size, n_channel,
              channels, target_kds, thresholds, mag, coi)
    jobs = [(share, *shared) for share in chunkify(chunk_ids, conf.ngpu_total)]
    log.info('Started dense prediction of {} in {:d} chunk(s), activation storage type {}.'.format(
        ", ".join(names), len(chunk_ids), conf['dense_prediction']['act_dtype']))
    cores = conf['ncores_per_node']
    if qu.batchjob_enabled():
        cores //= conf['ngpus_per_node']
    qu.batchjob_script(jobs, "predict_dense", n_cores=cores, suffix='_' + '_'.join(names), remove_jobfolder=True,
                       log=log, additional_flags="--gres=gpu:1")
    log.info('Finished dense prediction of {}'.format(", ".join(names)))


def get_myelin_cnn():
    """prediction.py:1047-1063: ``Predictor(torch.jit.load(mpath_myelin))`` with the default tiling of that loader."""
    return Predictor(global_params.config.mpath_myelin, strict_shapes=False, apply_softmax=True)


# -- multi-view networks (cell types) ---------------------------------------------------------------------------------------------
def naive_view_normalization_new(d):
    """prediction.py:1096-1097."""
    return d.astype(np.float32) / 255. - 0.5


def certainty_estimate(inp: np.ndarray, is_logit: bool = False) -> float:
    """prediction.py:1197-1227: one minus the entropy of the mean (pseudo-)probabilities over its maximum ln(C).  ``scipy.special
    .softmax`` (exp(x - max) / sum) and ``scipy.stats.entropy`` (normalise, then -sum p ln p with 0 ln 0 = 0) are restated in numpy, in
    the dtype of the input as there: scipy is no runtime dependency."""
    if not inp.ndim == 2:
        raise ValueError('Input is not two dimensional.')
    if is_logit:
        mx = np.max(inp, axis=1, keepdims=True)
        e = np.exp(inp - np.where(np.isfinite(mx), mx, 0))
        proba = e / np.sum(e, axis=1, keepdims=True)
    else:
        proba = inp
    proba = np.mean(proba, axis=0)
    entr_max = np.log(len(proba))
    pk = 1.0 * proba / np.sum(proba, axis=0, keepdims=True)
    with np.errstate(divide='ignore', invalid='ignore'):
        terms = np.where(pk > 0, -pk * np.log(pk), np.where(pk == 0, 0, -np.inf)).astype(pk.dtype)
    entr_norm = np.sum(terms, axis=0) / entr_max
    return 1 - entr_norm


def views_to_uint8(x: np.ndarray) -> np.ndarray:
    """Views that were normalised with ``naive_view_normalization_new`` back to the uint8 renderings they came from.  Only exact:
    ``u = rint((x + 0.5) 255)`` must reproduce every element of `x` bit for bit (views are always uint8 renderings; the device
    multiplies the integers and normalises in its epilogue), NotImplementedError otherwise."""
    x = np.asarray(x)
    if x.dtype != np.float32:
        raise NotImplementedError(f'views must be uint8 or float32 normalised uint8, got {x.dtype}')
    with np.errstate(invalid='ignore'):
        u = np.rint((x.astype(np.float64) + 0.5) * 255.)
    ok = np.isfinite(u).all() and u.min(initial=0) >= 0 and u.max(initial=0) <= 255
    if ok:
        u8 = u.astype(np.uint8)
        ok = np.array_equal(naive_view_normalization_new(u8), x)
    if not ok:
        raise NotImplementedError('float32 views that are not naive_view_normalization_new(uint8 views): the view network reads the '
                                  'uint8 renderings; pass those')
    return u8


class ViewSamples:
    """The internal input form of ``ViewModel.predict_proba``: the renderer's tensor ``views`` uint8 (n_loc, C, nb_views, H, W) (device or
    host) and ``table`` int32 (n_samples, D), the plane ``loc * nb_views + view`` of every slot of every sample."""

    def __init__(self, views, table):
        self.views, self.table = views, table


class _DeviceNet:
    """What the view models share: the weights of a spec (`weights`: a state dict, a module, or the path of a ``torch.jit`` file) as one
    float32 blob, the device, and the handle of the C model ``sd_<_net>_*`` that the subclass's ``_create(lib, blob, n_floats, dtype,
    out)`` makes."""

    _net = ''      # 'viewnet' / 'fcn'

    def __init__(self, spec, weights, act_dtype: str, bs: int, device):
        from .. import _dev as dv
        import ctypes as C
        if act_dtype not in ('f16', 'bf16'):
            raise ValueError("act_dtype must be 'f16' or 'bf16'")
        if isinstance(weights, (str, os.PathLike)):
            weights = torch.jit.load(os.fspath(weights), map_location='cpu')
        if hasattr(weights, 'state_dict'):
            weights = weights.state_dict()
        arrs = spec.weights_from_state_dict(weights)
        self.spec, self.act_dtype, self.bs = spec, act_dtype, self._bs(bs)
        self.dev = dv.device(device)
        blob = np.concatenate([a.ravel() for a in arrs]).astype(np.float32)
        h = C.c_void_p()
        with torch.cuda.device(self.dev):
            L.check(self._create(L.load(), blob.ctypes.data_as(C.POINTER(C.c_float)), blob.size, L.SD_F16 if act_dtype == 'f16' else L.SD_BF16,
                                 C.byref(h)), f'sd_{self._net}_create')
        self._h = h
        self._last = None      # the last launch set: the arguments of read_buffer behind the index, device tensors as they are

    def __del__(self):
        h, self._h = getattr(self, '_h', None), None
        if h:
            getattr(L.load(), f'sd_{self._net}_destroy')(h)

    @staticmethod
    def _bs(bs) -> int:
        bs = int(bs)
        if bs < 1:
            raise ValueError('bs must be positive')
        return bs

    @property
    def num_ops(self) -> int:
        return getattr(L.load(), f'sd_{self._net}_num_ops')(self._h)

    def _read_buffer(self, index: int) -> np.ndarray:
        """``sd_<_net>_read_buffer`` twice: for the dims, then for the data."""
        from .. import _dev as dv
        import ctypes as C
        if self._last is None:
            raise RuntimeError('read_buffer: no forward yet')
        name = f'sd_{self._net}_read_buffer'
        read = getattr(L.load(), name)
        args = (self._h, int(index), *(a.data_ptr() if isinstance(a, torch.Tensor) else a for a in self._last))
        dims = (C.c_int32 * 4)()
        L.check(read(*args, None, dims, dv.stream(self.dev)), name)
        out = np.empty(tuple(dims), dtype=np.float32)
        L.check(read(*args, out.ctypes.data_as(C.POINTER(C.c_float)), dims, dv.stream(self.dev)), name)
        return out


class ViewModel(_DeviceNet):
    """``InferenceModel`` of elektronn3 (prediction.py:999) for a view network given as a spec: ``predict_proba(inp, bs=None)`` with
    ``inp = views`` or ``(views, scalars)`` returns the float32 logits (n_samples, n_classes) -- the cell type path passes no normalising
    function, so "proba" are logits there too.  `weights`: a state dict, a module, or the path of a ``torch.jit`` file.  The views are
    uint8 (n_samples, C, D, H, W), a ``ViewSamples``, or float32 that ``views_to_uint8`` takes.  Deviations: DESIGN.md."""

    _net = 'viewnet'
    _entry = 'sd_viewnet_forward'      # the C entry of a launch set (EmbeddingModel: the one with the sample-tiled head)

    def __init__(self, spec, weights, act_dtype: str = 'f16', bs: int = 40, device=None):
        super().__init__(spec, weights, act_dtype, bs, device)

    def _create(self, lib, blob, n_floats, dtype, out):
        import ctypes as C
        spec = self.spec
        descs = (L.ViewNetLayerDesc * len(spec.layers))(*[L.ViewNetLayerDesc(*l) for l in spec.layers])
        sizes = spec.linear_sizes
        fc = (C.c_int32 * len(sizes))(*sizes)
        return lib.sd_viewnet_create(descs, len(spec.layers), fc, len(sizes) - 1, spec.in_channels, spec.n_scalar,
                                     0 if spec.act == 'relu' else 1, blob, n_floats, dtype, out)

    def _samples(self, views) -> 'ViewSamples':
        if isinstance(views, ViewSamples):
            v, t = views.views, views.table
        else:
            if isinstance(views, np.ndarray) and views.dtype == np.float32:
                views = views_to_uint8(views)
            v = views
            if getattr(v, 'ndim', 0) != 5:
                raise ValueError('views must be (n_samples, C, D, H, W)')
            t = np.arange(v.shape[0] * v.shape[2], dtype=np.int32).reshape(v.shape[0], v.shape[2])
        v = torch.from_numpy(np.ascontiguousarray(v)) if isinstance(v, np.ndarray) else v
        t = torch.from_numpy(np.ascontiguousarray(t)) if isinstance(t, np.ndarray) else t
        if not isinstance(v, torch.Tensor) or v.dtype != torch.uint8 or v.dim() != 5:
            raise ValueError('views must be a uint8 array / tensor (n_loc, C, nb_views, H, W)')
        if v.shape[1] != self.spec.in_channels:
            raise ValueError(f'views have {v.shape[1]} channels, the model takes {self.spec.in_channels}')
        if v.numel() == 0:
            raise ValueError('views are empty')
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or t.dim() != 2 or t.shape[0] < 1 or t.shape[1] < 1:
            raise ValueError('the sample table must be int32 (n_samples, D) with at least one sample')
        return ViewSamples(v.to(self.dev).contiguous(), t.to(self.dev).contiguous())

    def predict_proba(self, inp, bs: Optional[int] = None) -> np.ndarray:
        return self._forward(inp, bs).cpu().numpy()

    def _forward(self, inp, bs: Optional[int] = None) -> torch.Tensor:
        """``predict_proba`` with the logits left on the device."""
        from .. import _dev as dv
        views, scal = inp if isinstance(inp, (tuple, list)) else (inp, None)
        spec = self.spec
        bs = self.bs if bs is None else self._bs(bs)
        sm = self._samples(views)
        n, D = int(sm.table.shape[0]), int(sm.table.shape[1])
        n_loc, _, nb_views, H, W = (int(x) for x in sm.views.shape)
        spec.check_geometry(D, H, W)
        if spec.n_scalar:
            if scal is None:
                raise ValueError(f'the model takes {spec.n_scalar} scalars per sample')
            scal = torch.as_tensor(np.asarray(scal, dtype=np.float32) if not isinstance(scal, torch.Tensor) else scal)
            if tuple(scal.shape) != (n, spec.n_scalar):
                raise ValueError(f'scalars must be ({n}, {spec.n_scalar}), got {tuple(scal.shape)}')
            scal = scal.to(device=self.dev, dtype=torch.float32).contiguous()
        elif scal is not None and np.asarray(scal.cpu() if isinstance(scal, torch.Tensor) else scal).size:
            raise ValueError('the model takes no scalars')
        nb = min(bs, n)
        with torch.cuda.device(self.dev):
            ws = dv.scratch('sd_viewnet_workspace_bytes', self.dev, self._h, nb, D, H, W)
            logits = torch.empty((n, spec.n_classes), dtype=torch.float32, device=self.dev)
            flags = torch.zeros((-(-n // nb), 2), dtype=torch.int32, device=self.dev)
            for i, b in enumerate(range(0, n, nb)):
                e = min(b + nb, n)
                dv.call(self._entry, self.dev, self._h, sm.views, n_loc * nb_views, nb_views, H, W, sm.table[b:e], e - b, D,
                        scal[b:e] if spec.n_scalar else None, logits[b:e], ws, ws.numel(), flags[i])
            fl = flags.cpu().numpy()
        self._last = (ws, logits[b:e], e - b, D, H, W)
        if fl[:, 1].any():
            raise IndexError(f'sample table: an entry is outside [0, {n_loc * nb_views}) (n_loc * nb_views planes)')
        if fl[:, 0].any():
            raise L.ActivationOverflowError("fp16 activation storage overflowed in the view network: its logits are invalid; use "
                                            "act_dtype='bf16'")
        return logits

    def read_buffer(self, index: int) -> np.ndarray:
        """Debug: after ``predict_proba``, the stored output of layer `index` of the LAST launch set as float32 (planes, Ho, Wo, cout), or
        for ``index >= len(spec.layers)`` the output of Linear ``index - len(spec.layers)`` as (n_samples, out)."""
        out = self._read_buffer(index)
        return out if index < len(self.spec.layers) else out.reshape(out.shape[0], out.shape[3])


def get_celltype_model_e3(act_dtype: str = 'f16', n_classes: int = 7, n_scalar: int = 2):
    """prediction.py:985-1000: ``torch.jit.load(mpath_celltype_e3)`` -> state dict -> the view network (bs=40 as there)."""
    from ..cnn.viewnet_spec import CELLTYPE_CMN
    return ViewModel(CELLTYPE_CMN(n_classes, n_scalar), global_params.config.mpath_celltype_e3, act_dtype=act_dtype, bs=40)


# -- morphology embeddings from multi-views (the triplet network) ------------------------------------------------------------------------
def views2tripletinput(views):
    """prediction.py:1189-1194: (n, C, nb_views, H, W) -> float32 (n, C, 3, H, W), view 0 followed by two planes of ones."""
    first = np.asarray(views)[:, :, :1]
    ones = np.ones_like(first)
    return np.concatenate((first, ones, ones), axis=2).astype(np.float32)


class EmbeddingModel(ViewModel):
    """``InferenceModel`` around the ``TripletNet`` of cnn/cnn_atn.py:90-116 as reps/super_segmentation_helper.py:1803-1809 and
    reps/super_segmentation_object.py:3063-3069 call it, for the representation network given as a spec (``TNET_REP``): only ``z_0 =
    rep_net(x)`` is computed.  ``predict_proba(inp, bs=None)`` takes

    * uint8 views (n, C, H, W) -- what the module takes --, or float32 ones that ``views_to_uint8`` accepts,
    * the renderer's (n_loc, C, nb_views, H, W) tensor, host or device: view 0 of every location is read in place,
    * a ``ViewSamples`` whose table is (n, 1),
    * the reference's triple ``(x, y, z)``, of which `x` is used,

    and returns the float32 latents (n, z_dim); for the triple ``(None, None, latent, None, None)``, so that the reference's
    ``_, _, latent, _, _ = model.predict_proba(inp)`` works: the two distances and the latents of `y` and `z`, which the callers throw
    away, are not computed.  A launch set is `bs` planes; the default of 800 is the 40 x 20 planes of a cell type launch set and
    rests on no measurement.  The head runs sample-tiled (``sd_viewnet_embed``), with the bits of ``ViewModel``'s head."""
    _entry = 'sd_viewnet_embed'

    def __init__(self, spec, weights, act_dtype: str = 'f16', bs: int = 800, device=None):
        super().__init__(spec, weights, act_dtype=act_dtype, bs=bs, device=device)

    @property
    def tile_samples(self) -> int:
        """Samples per workgroup of the head kernel."""
        return L.load().sd_viewnet_embed_tile_samples(self._h)

    def _view0(self, views) -> 'ViewSamples':
        if isinstance(views, ViewSamples):
            t = views.table
            if getattr(t, 'ndim', 0) != 2 or t.shape[1] != 1:
                raise ValueError('the sample table of an embedding call must be (n, 1): one view per sample')
            return views
        if isinstance(views, np.ndarray) and views.dtype == np.float32:
            views = views_to_uint8(views)
        nd = getattr(views, 'ndim', 0)
        if nd == 4:
            return ViewSamples(views[:, :, None], np.arange(views.shape[0], dtype=np.int32).reshape(-1, 1))
        if nd == 5:
            return ViewSamples(views, (np.arange(views.shape[0], dtype=np.int32) * np.int32(views.shape[2])).reshape(-1, 1))
        raise ValueError('views must be (n, C, H, W) or (n_loc, C, nb_views, H, W)')

    def predict_proba(self, inp, bs: Optional[int] = None):
        triple = isinstance(inp, (tuple, list))
        if triple and len(inp) != 3:
            raise ValueError('a tuple input must be the triple (x, y, z) of the TripletNet')
        latent = self.predict_device(inp[0] if triple else inp, bs).cpu().numpy()
        return (None, None, latent, None, None) if triple else latent

    def predict_device(self, views, bs: Optional[int] = None) -> torch.Tensor:
        """The latents of `views` (any of the forms above but the triple) as a float32 device tensor (n, z_dim)."""
        return self._forward(self._view0(views), bs)

    def forward_samples(self, inp, bs: Optional[int] = None) -> np.ndarray:
        """``ViewModel.predict_proba`` -- any sample table, scalars -- through the tiled head."""
        return self._forward(inp, bs).cpu().numpy()


def get_tripletnet_model_e3(act_dtype: str = 'f16'):
    """prediction.py:1033-1044: ``torch.jit.load(mpath_tnet)`` -> state dict -> the representation network of cnn/cnn_atn.py (25 values)
    for the 128 x 256 window of the config.  A file whose first Linear takes another size is refused with both shapes in the message."""
    from ..cnn.viewnet_spec import TNET_REP
    return EmbeddingModel(TNET_REP(), global_params.config.mpath_tnet, act_dtype=act_dtype)


# -- glia probabilities from supervoxel views ---------------------------------------------------------------------------------------------
def glia_view_probas(logits: torch.Tensor) -> torch.Tensor:
    """float32 device logits (n, 2) -> float32 device probabilities (n, 2): the softmax of every row in float64, rounded once
    (``sd_glia_view_probas``).  A NaN or infinite logit is a ``ValueError``."""
    from .. import _dev as dv
    if not isinstance(logits, torch.Tensor) or not logits.is_cuda or logits.dtype != torch.float32 or logits.dim() != 2 or logits.shape[1] != 2:
        raise ValueError('glia_view_probas: logits must be a float32 device tensor (n, 2)')
    logits = logits.contiguous()
    n, dev = int(logits.shape[0]), logits.device
    probas = torch.empty((n, 2), dtype=torch.float32, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        dv.call('sd_glia_view_probas', dev, logits if n else None, n, probas if n else None, flag)
        if int(flag.cpu()[0]):
            raise ValueError('glia_view_probas: a logit is NaN or infinite')
    return probas


class GliaViewModel(ViewModel):
    """``InferenceModel(mpath_glia_e3, normalize_func=naive_view_normalization_new)`` (prediction.py:978-982) for the glia view network
    given as a spec (``GLIA_CMN``).  ``predict_proba(views, bs=None, apply_softmax=True)`` takes uint8 views (n, 1, 2, H, W), host or
    device, float32 ones that ``views_to_uint8`` accepts, or a ``ViewSamples``, and returns float32 (n, 2): the probabilities of neuron
    and glia.  The softmax is stated, not pinned (elektronn3 is not in the reference tree): the reference thresholds column 1 at
    ``glia_thresh``, which only makes sense for a probability.  ``apply_softmax=False`` gives the logits, the bits of a plain
    ``ViewModel`` run through the same head entry.  Every sample is two planes, so thousands of samples make one call: the head runs
    sample-tiled (``sd_viewnet_embed``); a launch set is `bs` samples, and the default of 400 (the 800 planes of an embedding launch
    set) rests on no measurement."""
    _entry = 'sd_viewnet_embed'

    def __init__(self, spec, weights, act_dtype: str = 'f16', bs: int = 400, device=None):
        if spec.n_classes != 2 or spec.n_scalar != 0:
            raise ValueError('GliaViewModel: the spec must have two classes and no scalars')
        super().__init__(spec, weights, act_dtype=act_dtype, bs=bs, device=device)

    def predict_device(self, views, bs: Optional[int] = None, apply_softmax: bool = True) -> torch.Tensor:
        """``predict_proba`` with the result left on the device."""
        if not isinstance(views, ViewSamples) and getattr(views, 'ndim', 0) == 5 and views.shape[0] == 0:
            if views.shape[1] != self.spec.in_channels:
                raise ValueError(f'views have {views.shape[1]} channels, the model takes {self.spec.in_channels}')
            return torch.zeros((0, 2), dtype=torch.float32, device=self.dev)
        logits = self._forward(views, bs)
        return glia_view_probas(logits) if apply_softmax else logits

    def predict_proba(self, views, bs: Optional[int] = None, apply_softmax: bool = True, verbose: bool = False) -> np.ndarray:
        return self.predict_device(views, bs, apply_softmax).cpu().numpy()


def get_glia_model_e3(act_dtype: str = 'f16'):
    """prediction.py:978-982: the glia view network with the weights of ``config.mpath_glia_e3``."""
    from ..cnn.viewnet_spec import GLIA_CMN
    return GliaViewModel(GLIA_CMN(), global_params.config.mpath_glia_e3, act_dtype=act_dtype)


# -- 2D semantic segmentation of multi-views (compartments) -------------------------------------------------------------------------
def semseg_views_to_uint8(x: np.ndarray) -> np.ndarray:
    """float32 views that are exactly ``u.astype(np.float32) / 255.`` of uint8 renderings `u` (what ``predict_views_semseg`` hands to
    the model, reps/super_segmentation_helper.py:1372) back to `u`; anything else is a NotImplementedError: the network reads the uint8
    renderings and applies 1 / 255 in its first epilogue."""
    x = np.asarray(x)
    if x.dtype != np.float32:
        raise NotImplementedError(f'views must be uint8 or float32 uint8 / 255, got {x.dtype}')
    with np.errstate(invalid='ignore'):
        u = np.rint(x.astype(np.float64) * 255.)
    ok = np.isfinite(u).all() and u.min(initial=0) >= 0 and u.max(initial=0) <= 255
    if ok:
        u8 = u.astype(np.uint8)
        ok = np.array_equal(u8.astype(np.float32) / 255., x)
    if not ok:
        raise NotImplementedError('float32 views that are not uint8 views / 255: the semantic-segmentation network reads the uint8 '
                                  'renderings; pass those')
    return u8


class SemsegViewModel(_DeviceNet):
    """``InferenceModel`` of elektronn3 (prediction.py:1003-1030) for an FCN given as a spec (syconn_amd/cnn/fcn_spec.py).
    ``predict_proba(views (N, C, H, W))`` returns the float32 logits (N, n_class, H, W) -- the reference passes no normalising
    function and takes the argmax, which a softmax would not change --; ``predict_labels(views (n_loc, C, nb_views, H, W))`` reads
    the renderer's tensor in place, host or device, and returns the uint8 labels (n_loc, 1, nb_views, H, W) of
    ``predict_views_semseg`` as the same kind (array or device tensor).  `weights`: a state dict, a module, or the path of a
    ``torch.jit`` file.  Views are uint8, or float32 that ``semseg_views_to_uint8`` takes.  A launch set holds at most `bs` planes and
    at most ``max_workspace_bytes`` of workspace."""

    max_workspace_bytes = 4 << 30
    _net = 'fcn'

    def __init__(self, spec, weights, act_dtype: str = 'f16', bs: int = 10, device=None):
        super().__init__(spec, weights, act_dtype, bs, device)

    def _create(self, lib, blob, n_floats, dtype, out):
        import ctypes as C
        spec = self.spec
        flat = [c for b in spec.blocks for c in b]
        blocks, lens = (C.c_int32 * len(flat))(*flat), (C.c_int32 * 5)(*[len(b) for b in spec.blocks])
        return lib.sd_fcn_create(spec.in_channels, blocks, lens, spec.dec_last, spec.n_class, blob, n_floats, dtype, out)

    def _views(self, views, ndim: int) -> torch.Tensor:
        if isinstance(views, np.ndarray) and views.dtype == np.float32:
            views = semseg_views_to_uint8(views)
        v = torch.from_numpy(np.ascontiguousarray(views)) if isinstance(views, np.ndarray) else views
        shape = '(N, C, H, W)' if ndim == 4 else '(n_loc, C, nb_views, H, W)'
        if not isinstance(v, torch.Tensor) or v.dtype != torch.uint8 or v.dim() != ndim:
            raise ValueError(f'views must be a uint8 array / tensor {shape}')
        if ndim == 4:
            v = v[:, :, None]
        if v.shape[1] != self.spec.in_channels:
            raise ValueError(f'views have {v.shape[1]} channels, the model takes {self.spec.in_channels}')
        if v.numel() == 0:
            raise ValueError('views are empty')
        self.spec.check_geometry(int(v.shape[3]), int(v.shape[4]))
        return v.to(self.dev).contiguous()

    def _forward(self, v: torch.Tensor, bs: Optional[int], want_logits: bool):
        from .. import _dev as dv
        bs = self.bs if bs is None else self._bs(bs)
        n_loc, _, nb_views, H, W = (int(x) for x in v.shape)
        n = n_loc * nb_views
        per_plane = int(L.load().sd_fcn_workspace_bytes(self._h, 1, H, W))
        nb = max(1, min(bs, n, self.max_workspace_bytes // max(per_plane, 1)))
        with torch.cuda.device(self.dev):
            ws = dv.scratch('sd_fcn_workspace_bytes', self.dev, self._h, nb, H, W)
            labels = torch.empty((n, H, W), dtype=torch.uint8, device=self.dev)
            logits = torch.empty((n, self.spec.n_class, H, W), dtype=torch.float32, device=self.dev) if want_logits else None
            flags = torch.zeros((-(-n // nb), 1), dtype=torch.int32, device=self.dev)
            for i, b in enumerate(range(0, n, nb)):
                e = min(b + nb, n)
                dv.call('sd_fcn_forward', self.dev, self._h, v, n, nb_views, H, W, b, e - b, labels[b:e], logits[b:e] if want_logits else None, ws,
                        ws.numel(), flags[i])
            fl = flags.cpu().numpy()
        self._last = (ws, logits[b:e] if want_logits else None, e - b, H, W)
        if fl.any():
            raise L.ActivationOverflowError("fp16 activation storage overflowed in the semantic-segmentation network: its labels are "
                                            "invalid; use act_dtype='bf16'")
        return labels.view(n_loc, 1, nb_views, H, W), logits

    def predict_proba(self, views, bs: Optional[int] = None, verbose: bool = False) -> np.ndarray:
        _, logits = self._forward(self._views(views, 4), bs, True)
        return logits.cpu().numpy()

    def predict_labels(self, views, bs: Optional[int] = None):
        labels, _ = self._forward(self._views(views, 5), bs, False)
        return labels if isinstance(views, torch.Tensor) else labels.cpu().numpy()

    def read_buffer(self, index: int) -> np.ndarray:
        """Debug: after a forward, the stored output of op `index` of the LAST launch set as float32 (planes, h, w, c); the last op's are
        the logits (planes, n_class, H, W) (``predict_proba`` only)."""
        return self._read_buffer(index)


def get_semseg_spiness_model(act_dtype: str = 'f16', n_class: int = 5):
    """prediction.py:1003-1015: ``torch.jit.load(mpath_spiness)`` -> state dict -> the FCN (cnn/cnn_spineseg.py:28-29)."""
    from ..cnn.fcn_spec import FCN_VGG13
    return SemsegViewModel(FCN_VGG13(n_class), global_params.config.mpath_spiness, act_dtype=act_dtype)


def get_semseg_axon_model(act_dtype: str = 'f16', n_class: int = 6):
    """prediction.py:1018-1030: ``torch.jit.load(mpath_axonsem)`` -> state dict -> the FCN (cnn/cnn_axonseg.py:34-35)."""
    from ..cnn.fcn_spec import FCN_VGG13
    return SemsegViewModel(FCN_VGG13(n_class), global_params.config.mpath_axonsem, act_dtype=act_dtype)
