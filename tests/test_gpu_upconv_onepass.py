"""The one-pass row up-convolution (`k_upconv_rows1`: input fragments loaded once, weights streamed through two LDS slots)
against the forms it replaces and against the float64 one-op reference of tests/_unet_step_ref.py.

A case = one forward of a semseg_spine variant under SD_KEEP_ALL=1 whose tile is chosen so that the up-convolution under test
gets the source box the case names.  SD_UPCONV_ONEPASS=1 selects the one-pass form at every launch-set size, =0 the old forms
(the default rule selects it only from the headline launch-set size on).  Per case, for the up-convolution under test:
  1. its output buffer (tile 0) and the logits of ALL tiles equal those of the SD_UPCONV_ONEPASS=0 run bit for bit,
  2. the output lies within the rule of the reference module (half a storage ulp + c 2^-24 S) of the float64 reference
     computed from the device's own input buffer,
  3. `op_kernels()` names the one-pass form for it (and the old form in the =0 run).
Source boxes: 3x5x7 (105 voxels: less than one 256-voxel group, a partial wave, idle waves), 2x9x33 (594: no multiple of 32,
rows wrap inside a wave), 4x8x40 (1280 = 5 groups; run once with one group per workgroup and once with
SD_UPCONV_ONEPASS_WGS=2, i.e. 3 and 2 groups per persistent workgroup and a clamped prefetch behind the last one).
96 -> 48 channels is not selected for the one-pass form, so it has no case here.
"""
import functools

import pytest
import torch

from oracle.unet_ref import build_unet
from syconn_amd.plan import plan_from_model

import _unet_step_ref as R

pytestmark = pytest.mark.gpu

# layer -> (overrides of semseg_spine, input channels of the up-convolution, kz, tile extent per source extent (z, y, x))
LAYERS = {
    '128to64-kz2': (dict(), 128, 2, (2, 4, 4)),
    '128to64-kz1': (dict(planar_blocks=(0, 1, 2)), 128, 1, (1, 4, 4)),
    '256to128-kz1': (dict(), 256, 1, (2, 8, 8)),
}
NEW = {128: 'k_upconv_rows<NCH=8,NTAB=4,one pass>', 256: 'k_upconv_rows<NCH=16,NTAB=8,one pass>'}
BOXES = [((3, 5, 7), None), ((2, 9, 33), None), ((4, 8, 40), None), ((4, 8, 40), 2)]


@functools.lru_cache(maxsize=None)
def _net(layer):
    return build_unet('semseg_spine', seed=5, **LAYERS[layer][0])


@functools.lru_cache(maxsize=None)
def _ref(layer, act):
    ops, blob, _ = plan_from_model(_net(layer))
    return R.StepRef(ops, blob, act)


def _forward(dm, x, gpu):
    from syconn_amd import _lib as L
    if x.shape[0] == 1:
        return dm.forward(x[0].to(gpu), L.SD_OUT_LOGITS_F32).cpu()[None]
    return dm.forward_batch(x.to(gpu), L.SD_OUT_LOGITS_F32).cpu()


@pytest.mark.parametrize('batch', [1, 3])
@pytest.mark.parametrize('act', ['bf16', 'f16'])
@pytest.mark.parametrize('box,wgs', BOXES, ids=['3x5x7', '2x9x33', '4x8x40', '4x8x40-2wgs'])
@pytest.mark.parametrize('layer', list(LAYERS))
def test_one_pass_step(gpu, monkeypatch, layer, box, wgs, act, batch):
    from syconn_amd.engine import DenseModel
    _, cin, kz, mul = LAYERS[layer]
    monkeypatch.setenv('SD_KEEP_ALL', '1')
    if wgs:
        monkeypatch.setenv('SD_UPCONV_ONEPASS_WGS', str(wgs))
    sr = _ref(layer, act)
    unit = next(u for u in sr.units() if u[0] == 'upconv' and sr.ops[u[1]].cin0 == cin)
    i, d = unit[1], sr.ops[unit[1]]
    assert d.kz == kz and unit[2] < 0
    tile = tuple(b * m for b, m in zip(box, mul))
    g = torch.Generator().manual_seed(11 * box[2] + batch)
    x = torch.randint(0, 256, (batch, *tile), generator=g, dtype=torch.uint8)
    dm = DenseModel(_net(layer), act_dtype=act, device=gpu)

    monkeypatch.setenv('SD_UPCONV_ONEPASS', '0')
    logits_old = _forward(dm, x, gpu)
    sym_old = dm.op_kernels()[i][1]
    out_old = dm.read_buffer(d.dst).cpu().clone()
    assert 'one pass' not in sym_old and 'k_upconv' in sym_old, sym_old

    monkeypatch.setenv('SD_UPCONV_ONEPASS', '1')
    logits_new = _forward(dm, x, gpu)
    sym_new = dm.op_kernels()[i][1]
    assert not dm.overflowed()
    assert NEW[cin] in sym_new.replace(f'<{act},', '<'), (sym_new, sym_old)          # 3.
    src = dm.read_buffer(d.src0).cpu()
    assert tuple(src.shape[1:]) == box, (src.shape, box)
    out_new = dm.read_buffer(d.dst).cpu()

    assert out_new.dtype == out_old.dtype and out_new.shape == out_old.shape
    assert torch.equal(out_new.view(torch.int32), out_old.view(torch.int32)), \
        f'{int((out_new.view(torch.int32) != out_old.view(torch.int32)).sum())} elements differ from the old form'     # 1.
    assert torch.equal(logits_new.view(torch.int32), logits_old.view(torch.int32)), 'logits of some tile differ'

    res = sr.compute(unit, src.to(torch.float64))                                    # 2.
    nbad, worst, ratio, _ = sr.check(out_new.to(torch.float64), res)
    print(f'ONEPASS {layer} {box}x{batch} {act} wgs {wgs}: {sym_new} ratio {ratio:.3f}')
    assert nbad == 0, f'{nbad} of {out_new.numel()} elements over the rule, worst {ratio:.1f} x the allowed difference at {worst}'


def test_whole_net_labels_equal(gpu, monkeypatch):
    """semseg_spine, 16 x 32 x 32, two tiles: forward_labels_batch returns equal bytes with the switch on and off."""
    from syconn_amd.engine import DenseModel
    dm = DenseModel(build_unet('semseg_spine', seed=3, final_scale=8.0), act_dtype='bf16', device=gpu)
    x = torch.randint(0, 256, (2, 16, 32, 32), generator=torch.Generator().manual_seed(2), dtype=torch.uint8).to(gpu)
    ids, thr = list(range(1, dm.out_channels)), [127.5] * (dm.out_channels - 1)
    monkeypatch.setenv('SD_UPCONV_ONEPASS', '0')
    old = dm.forward_labels_batch(x, ids, thr).cpu().clone()
    assert not any('one pass' in s for _, s in dm.op_kernels())
    monkeypatch.setenv('SD_UPCONV_ONEPASS', '1')
    new = dm.forward_labels_batch(x, ids, thr).cpu()
    assert sum('one pass' in s for _, s in dm.op_kernels()) == 2, dm.op_kernels()
    assert new.dtype == old.dtype and new.shape == old.shape and torch.equal(new, old)
    assert old.unique().numel() > 1
