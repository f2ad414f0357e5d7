"""Every layer form of the bf16 / f16 U-Net plans against the float64 reference of that ONE op (tests/_unet_step_ref.py).

Per case: a `DenseModel` under SD_KEEP_ALL=1 (every activation buffer is stored) plus the A/B switch the case names, one
forward, `op_kernels()` for the kernel symbol that computed each op; then for every op (or the ops whose symbol matches the
case's filter) the device's own INPUT buffers go through the float64 reference of that op and the result is compared with
the device's OUTPUT buffer under the rule of the reference module: half a storage ulp plus c 2^-24 S, pooling exact.  No
earlier layer's rounding enters.  With a batch the buffers of tile 0 are checked (`read_buffer` reads tile 0:
test_read_buffer_after_batch_is_tile_0).

Every case asserts through `op_kernels()` that the form it is named after really ran; a session-wide collector gathers the
symbols that were checked and the last test compares it with SYMBOLS, the hand-written list of what the launchers
(`launch_conv_knt`, `launch_upconv_t`, `launch_first`, `launch_pool`, `launch_final`, `launch_groupnorm`) can choose for
these two storage types outside the fused forms.  A label is the kernel symbol without its storage type, plus ' +pool' /
' +final' for an op computed in that launch's epilogue.

The final layer runs as a launch of its own behind a GroupNorm (mivcsj) and in the epilogue of the last convolution
otherwise ('+final'; under SD_KEEP_ALL the streaming level-0 decoder is off, so that holds for every tile height).

Not readable under SD_KEEP_ALL, pinned through their bit-identity tests in test_gpu_unet.py to forms checked here: the first
convolution inside the second (MODE=1 / 5), the deferred GroupNorm apply (MODE=2, `k_gn_finalize` alone, `k_gn_stats +
k_gn_finalize`), `k_dec0`.  Left out of SYMBOLS, with the reason, in NOT_COVERED.
"""
import functools
import json
import os
import re
import subprocess
import sys

import pytest
import torch

from oracle.unet_ref import build_cnn3, build_unet
from syconn_amd.plan import plan_from_model

import _unet_step_ref as R

pytestmark = pytest.mark.gpu
ACTS = ('bf16', 'f16')

CONV = 'k_conv_mfma<%s,NT=%d,WAVES=%d,NSLOT=%d,MT=%d,MODE=0>'


def _c(k, nt, waves, nslot, mt=2):
    return CONV % (k, nt, waves, nslot, mt)


# what the launchers can choose (storage type dropped: every case runs for both)
SYMBOLS = [
    # launch_conv_knt, small launch sets: 4 waves, resident weights where they fit 80 KiB, else streamed
    _c('1x3x3', 1, 4, 2), _c('1x3x3', 2, 4, 2), _c('1x3x3', 2, 4, 0), _c('1x3x3', 3, 4, 0),
    _c('3x3x3', 1, 4, 2), _c('3x3x3', 1, 4, 0), _c('3x3x3', 2, 4, 0), _c('3x3x3', 3, 4, 0),
    # ... 8 waves: resident weights (level 0), streamed, the 4-tile 3x3x3 form, the planar 4-tile form, the ring form
    _c('1x3x3', 1, 8, 2), _c('1x3x3', 2, 8, 2), _c('3x3x3', 1, 8, 0), _c('3x3x3', 3, 8, 0),
    _c('3x3x3', 2, 8, 0, 4), _c('3x3x3', 2, 8, 0), _c('1x3x3', 2, 4, 0, 4), _c('1x3x3', 2, 8, 0),
    _c('1x3x3', 3, 8, -3), _c('1x3x3', 3, 8, 0),
    # epilogue work of a convolution launch
    '+pool', '+final',
    # launch_first
    'k_conv_first<uint8 input, bf16 MFMA on the exact values>', 'k_conv_first<uint8 input, f32 MFMA chain>',
    'k_conv_first<float32 input, f32 MFMA chain>',
    # launch_upconv_t
    'k_upconv_rows<NCH=2,NTAB=1>', 'k_upconv_rows<NCH=3,NTAB=2>', 'k_upconv_rows<NCH=4,NTAB=2>',
    'k_upconv_rows<NCH=4,NTAB=2,LDS weights>', 'k_upconv_rows<NCH=6,NTAB=3>', 'k_upconv_rows<NCH=6,NTAB=3,LDS weights>',
    'k_upconv_rows<NCH=8,NTAB=4,LDS weights>', 'k_upconv_rows<NCH=12,NTAB=6,LDS weights>',
    'k_upconv_rows<NCH=16,NTAB=8,LDS weights,G=2>', 'k_upconv_rows<NCH=24,NTAB=12,LDS weights,G=6>', 'k_upconv_mfma',
    # launch_pool, launch_final, launch_groupnorm
    'k_maxpool', 'k_final_mfma / k_final', 'k_gn_finalize + k_gn_apply', 'k_gn_stats + k_gn_finalize + k_gn_apply',
]
NOT_COVERED = {
    'k_final (scalar)': 'behind the same symbol as k_final_mfma; taken from 481 padded channels on, which no network has',
    'k_conv_mfma 3x3x3,NT=2,NSLOT=2 / 3x3x3,NT=3,NSLOT=2 / 1x3x3,NT=3,NSLOT=2 / 1x3x3,NT=1,NSLOT=0':
        'the resident-weight rule (80 / 96 KiB of LDS) admits them only for 16 input channels (NT >= 2) or more than 128 (NT = 1): '
        'no network of the path has such a layer',
    'k_conv_mfma 3x3x3,NT=1,WAVES=8,NSLOT=2':
        'a 16 -> 32 channel 3x3x3 layer needs 95.5 KiB + parameters, just over the 96 KiB rule; the 150 KiB rule applies from 2^20 '
        'voxels per tile AT THAT LAYER on, i.e. level-0 tiles of 4 M voxels (the layer runs as NSLOT=0, which is checked)',
}

_checked = {}        # label -> {act: dict(n, worst c, one-step share)}


@functools.lru_cache(maxsize=None)
def _net(name):
    if name == 'cnn3':
        return build_cnn3(0)
    if name == 'myelin3x16':
        return build_unet('myelin', seed=1, n_blocks=3, start_filts=16)
    if name == 'myelin2x24':      # 48 -> 24 channels: the <NCH=3,NTAB=2> up-convolution
        return build_unet('myelin', seed=2, n_blocks=2, start_filts=24)
    if name == 'mivcsj_neg':      # half of the GroupNorm weights negative
        m = build_unet('mivcsj', seed=9)
        g = torch.Generator().manual_seed(1)
        with torch.no_grad():
            for k, v in m.state_dict().items():
                if '.norm' in k and k.endswith('.weight'):
                    v.mul_((torch.randint(0, 2, v.shape, generator=g) * 2 - 1).to(v.dtype))
        return m
    return build_unet(name, seed=3)


@functools.lru_cache(maxsize=None)
def _ref(name, act):
    ops, blob, _ = plan_from_model(_net(name))
    return R.StepRef(ops, blob, act)


def _input(shape, seed):
    """uint8 tile(s) holding all 256 values (from 256 voxels on)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(0, 256, shape, generator=g, dtype=torch.uint8)
    flat = x.reshape(-1)
    n = min(256, flat.numel())
    flat[torch.randperm(flat.numel(), generator=g)[:n]] = torch.arange(n, dtype=torch.int64).to(torch.uint8)
    return x


def _label(sym):
    return re.sub(r'<(bf16|f16),', '<', sym)


def _block_pos(label, idx, shape, d):
    """position of output element (c, z, y, x) inside the block of the form that computed it."""
    c, z, y, x = idx
    m = re.match(r'k_conv_mfma<(\d)x3x3,NT=(\d+),WAVES=(\d+),NSLOT=(-?\d+),MT=(\d+)', label)
    if m:
        kz, nt, waves, _, mt = (int(v) for v in m.groups())
        bz, by = ((waves // 4) * mt, 8) if kz == 3 else (1, waves * 2 * mt)
        return f'block {bz}x{by}x16 at (z,y,x) = ({z % bz},{y % by},{x % 16}), channel tile {c // 32} of {nt} per workgroup'
    if label.startswith('k_conv_first'):
        bz, by = (2, 8) if d.kz == 3 else (1, 16)
        return f'block {bz}x{by}x16 at ({z % bz},{y % by},{x % 16})'
    if label.startswith('k_upconv'):
        src = ((z // d.kz) * (shape[2] // 2) + y // 2) * (shape[3] // 2) + x // 2
        per = 256 if 'mfma' in label else 128
        return f'tap ({z % d.kz},{y % 2},{x % 2}), source voxel {src % per} of its {per}-voxel workgroup'
    return f'voxel {(z * shape[2] + y) * shape[3] + x} % 256 = {((z * shape[2] + y) * shape[3] + x) % 256}'


def run_case(gpu, monkeypatch, act, net, tile, batch=1, env=(), only=None, expect=(), inp='u8', seed=0):
    """Steps 1-6 of the module docstring.  Returns the set of labels checked."""
    from syconn_amd import _lib as L
    from syconn_amd.engine import DenseModel
    monkeypatch.setenv('SD_KEEP_ALL', '1')
    for k in env:
        monkeypatch.setenv(k, '1')
    sr = _ref(net, act)
    dm = DenseModel(_net(net), act_dtype=act, device=gpu)
    raw = _input((batch, *tile), seed + 17 * tile[0] + tile[2])
    xin = raw if inp == 'u8' else raw.to(torch.float32) / 255.
    if batch == 1:
        logits = dm.forward(xin[0].to(gpu), L.SD_OUT_LOGITS_F32).cpu()
    else:
        logits = dm.forward_batch(xin.to(gpu), L.SD_OUT_LOGITS_F32)[0].cpu()
    ks = dm.op_kernels()
    assert not dm.overflowed()
    seen, failures = set(), []
    bufs = {}

    def buf(b):
        if b not in bufs:
            bufs[b] = dm.read_buffer(b).cpu().to(torch.float64)
        return bufs[b]

    for unit in sr.units():
        kind, i, g = unit
        d = sr.ops[i]
        e, sym = ks[i]
        assert e >= 0 and sym, (i, ks[i])
        label = _label(sym)
        labels = [label]
        if kind == 'pool' and e != i:
            labels = ['+pool', label]
        if kind == 'final' and e != i:
            labels = ['+final', label]
        if g >= 0:
            labels.append(_label(ks[g][1]))
        if only is not None and not any(re.search(only, s) for s in labels):
            continue
        form = None
        if kind == 'conv' and d.src0 == 0:
            form = 'u8_mfma' if 'exact values' in label else 'f32_chain'
            x0 = xin[0]
        else:
            x0 = buf(d.src0)
        x1 = buf(d.src1) if (kind == 'conv' and d.src1 >= 0) else None
        region = tuple(buf(sr.ops[g].src1).shape[1:]) if (g >= 0 and sr.ops[g].src1 >= 0) else None
        res = sr.compute(unit, x0, x1, form=form, region=region)
        dev = logits.to(torch.float64) if kind == 'final' else buf(d.dst)
        if region is not None:
            dev = dev[:, :region[0], :region[1], :region[2]]
        nbad, worst, ratio, diff = sr.check(dev, res)
        seen.update(labels)
        # what section 5 of the issue asks to write down: (|dev - ref| - ulp_s / 2) / (2^-24 S), one-step share
        stat = ''
        if res['kind'] not in ('pool', 'gn'):
            ref = res['ref']
            half = (R.ulp_f32(ref.abs()) if kind == 'final' else R.ulp_s(ref.abs(), act)) / 2
            cobs = float(((diff - half) / (2.0 ** -24 * res['S'].clamp_min(1e-300))).max())
            if kind != 'final':
                # (where the storage step dominates the accumulation term: next to zero a value may be many of its own tiny
                # steps away and still within c 2^-24 S)
                rr = R.round_storage(ref, act)
                u = R.ulp_s(torch.maximum(rr.abs(), dev.abs()), act)
                steps = torch.where(u >= 8 * R.C[act] * 2.0 ** -24 * res['S'], (dev - rr).abs() / u, torch.zeros_like(u))
                share, most = float((steps > 0).double().mean()), float(steps.max())
            else:
                share, most = 0.0, 0.0
            stat = f'c_obs {cobs:.2f} one-step share {share:.2e} max steps {most:.1f}'
            for s in labels[:1] if labels[0].startswith('+') else labels:
                rec = _checked.setdefault(s, {}).setdefault(act, dict(n=0, c=-1e9, share=0.0, steps=0.0))
                rec['n'] += 1
                rec['c'], rec['share'], rec['steps'] = max(rec['c'], cobs), max(rec['share'], share), max(rec['steps'], most)
        else:
            for s in labels:
                _checked.setdefault(s, {}).setdefault(act, dict(n=0, c=-1e9, share=0.0, steps=0.0))['n'] += 1
        print(f'STEPSTAT {act} {net} {tile}x{batch} op {i} {" | ".join(labels)} ratio {ratio:.3f} {stat}')
        if nbad:
            idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(worst), dev.shape))
            failures.append(f'op {i} [{" | ".join(labels)}]: {nbad} of {dev.numel()} elements over the rule; worst at channel '
                            f'{idx[0]}, (z,y,x) = {idx[1:]} of {tuple(dev.shape[1:])}: {_block_pos(label, idx, dev.shape, d)}; '
                            f'dev {float(dev[idx]):.6g} ref {float(res["ref"][idx]):.6g}, {ratio:.1f} x the allowed difference')
    assert not failures, f'{net} {act} tile {tile} x {batch} {sorted(env)}:\n' + '\n'.join(failures)
    for s in expect:
        assert s in seen, f'{net} {tile} x {batch} {sorted(env)}: form {s} did not run; ran {sorted(seen)}'
    return seen


def test_read_buffer_after_batch_is_tile_0(gpu, monkeypatch):
    from syconn_amd import _lib as L
    from syconn_amd.engine import DenseModel
    monkeypatch.setenv('SD_KEEP_ALL', '1')
    dm = DenseModel(_net('myelin3x16'), act_dtype='bf16', device=gpu)
    x = _input((3, 5, 17, 19), 3).to(gpu)
    dm.forward(x[0], L.SD_OUT_LOGITS_F32)
    single = [dm.read_buffer(b).clone() for b in range(1, dm.info['n_buffers'])]
    dm.forward_batch(x, L.SD_OUT_LOGITS_F32)
    for b, want in zip(range(1, dm.info['n_buffers']), single):
        assert torch.equal(dm.read_buffer(b), want), b
    assert not torch.equal(x[0], x[1])


SMALL_TILES = [(1, 1, 1), (2, 3, 5), (3, 16, 2), (1, 40, 33), (5, 17, 50), (13, 27, 29), (9, 35, 37)]
SMALL_EXPECT = {      # the forms every tile of these launch sets selects (verified on the device, not by arithmetic)
    'myelin3x16': (_c('1x3x3', 1, 4, 2), _c('3x3x3', 1, 4, 2), '+pool', '+final', 'k_upconv_rows<NCH=2,NTAB=1>'),
    'semseg_spine': (_c('1x3x3', 1, 4, 2), _c('3x3x3', 2, 4, 0), _c('1x3x3', 2, 4, 0), '+pool', '+final',
                     'k_upconv_rows<NCH=4,NTAB=2,LDS weights>', 'k_upconv_rows<NCH=8,NTAB=4,LDS weights>', 'k_upconv_mfma'),
    'syntype': (_c('1x3x3', 1, 4, 2), _c('3x3x3', 2, 4, 0), '+pool', '+final', 'k_upconv_mfma'),
    'semseg_axon': (_c('1x3x3', 2, 4, 2), _c('3x3x3', 3, 4, 0), _c('1x3x3', 3, 4, 0), '+pool', '+final',
                    'k_upconv_rows<NCH=6,NTAB=3,LDS weights>', 'k_upconv_rows<NCH=12,NTAB=6,LDS weights>', 'k_upconv_mfma'),
    'mivcsj': (_c('1x3x3', 2, 4, 2), _c('3x3x3', 3, 4, 0), 'k_final_mfma / k_final', 'k_gn_finalize + k_gn_apply',
               'k_gn_stats + k_gn_finalize + k_gn_apply'),
    'cnn3': (_c('3x3x3', 1, 4, 2), 'k_conv_first<uint8 input, f32 MFMA chain>'),
}


@pytest.mark.parametrize('act', ACTS)
@pytest.mark.parametrize('tile', SMALL_TILES, ids=lambda t: 'x'.join(map(str, t)))
@pytest.mark.parametrize('net', list(SMALL_EXPECT))
def test_all_ops_small_launch_sets(gpu, monkeypatch, net, tile, act):
    """Every op of six networks on tiles where every voxel is a border voxel, D = 1, W < 16, odd extents through ceil-mode
    pooling and crop, and extents one above / below a multiple of the block extents (2/4/8 x 8 x 16, 1 x 16/32 x 16)."""
    run_case(gpu, monkeypatch, act, net, tile, expect=SMALL_EXPECT[net])


@pytest.mark.parametrize('act', ACTS)
@pytest.mark.parametrize('net,tile,batch,expect', [
    ('semseg_spine', (8, 129, 129), 1, _c('1x3x3', 1, 8, 2)),        # 133 k voxels, H / W one past a multiple of 32 / 16
    ('semseg_spine', (12, 129, 129), 1, _c('1x3x3', 1, 8, 2)),       # 540 blocks: more than the 512 the persistent grid holds
    ('semseg_axon', (8, 129, 129), 1, _c('1x3x3', 2, 8, 2)),
    ('myelin3x16', (9, 65, 49), 20, _c('1x3x3', 1, 8, 2)),           # 16 filters, 20 tiles
], ids=['spine', 'spine-blockloop', 'axon', 'myelin3x16'])
def test_eight_wave_resident_weight_forms(gpu, monkeypatch, net, tile, batch, expect, act):
    run_case(gpu, monkeypatch, act, net, tile, batch=batch, only=r'WAVES=8,NSLOT=2', expect=(expect,))


@pytest.mark.parametrize('act', ACTS)
@pytest.mark.parametrize('net,tile,batch,only,expect', [
    ('myelin3x16', (9, 65, 49), 20, r'3x3x3,NT=1,WAVES=8,NSLOT=0', _c('3x3x3', 1, 8, 0)),      # the merge convolution of level 1
    ('semseg_axon', (9, 65, 65), 16, r'3x3x3,NT=3,WAVES=8', _c('3x3x3', 3, 8, 0)),              # level 1: 9 x 33 x 33 x 16 tiles
], ids=['NT1', 'NT3'])
def test_eight_wave_streamed_3x3x3_forms(gpu, monkeypatch, net, tile, batch, only, expect, act):
    run_case(gpu, monkeypatch, act, net, tile, batch=batch, only=only, expect=(expect,))


@pytest.mark.parametrize('act', ACTS)
@pytest.mark.parametrize('mt2', [False, True], ids=['MT4', 'SD_MT2'])
@pytest.mark.parametrize('d', [13, 15])
def test_four_tile_3x3x3_form_and_partner(gpu, monkeypatch, d, mt2, act):
    """64-channel 3x3x3 layers of level 1 at d x 73 x 73 x 4 tiles (ragged z that the z rule accepts, odd y / x)."""
    run_case(gpu, monkeypatch, act, 'semseg_spine', (d, 145, 145), batch=4, env=('SD_MT2',) if mt2 else (),
             only=r'3x3x3,NT=2,WAVES=8', expect=(_c('3x3x3', 2, 8, 0, 2 if mt2 else 4),))


@pytest.mark.parametrize('act', ACTS)
@pytest.mark.parametrize('no_p4', [False, True], ids=['planar4', 'SD_NO_PLANAR4'])
def test_planar_four_tile_form_and_partner(gpu, monkeypatch, no_p4, act):
    """128-channel planar layers of level 2 at 30 x 33 x 31 x 9 tiles."""
    run_case(gpu, monkeypatch, act, 'semseg_spine', (60, 130, 122), batch=9, env=('SD_NO_PLANAR4',) if no_p4 else (),
             only=r'1x3x3,NT=2,WAVES=[48],NSLOT=0', expect=(_c('1x3x3', 2, 8, 0) if no_p4 else _c('1x3x3', 2, 4, 0, 4),))


@pytest.mark.parametrize('act', ACTS)
@pytest.mark.parametrize('no_ring', [False, True], ids=['ring', 'SD_NO_RING'])
def test_ring_form_and_partner(gpu, monkeypatch, no_ring, act):
    """192-channel planar layers of semseg_axon's level 2 at 15 x 33 x 31 x 5 tiles.  Planar NT=3 layers take the 8-wave
    forms only under SD_PLANAR_NT3_BIG (launch_conv_knt), so the case sets it."""
    run_case(gpu, monkeypatch, act, 'semseg_axon', (30, 130, 122), batch=5,
             env=('SD_PLANAR_NT3_BIG',) + (('SD_NO_RING',) if no_ring else ()), only=r'1x3x3,NT=3,WAVES=8',
             expect=(_c('1x3x3', 3, 8, 0) if no_ring else _c('1x3x3', 3, 8, -3),))


@pytest.mark.parametrize('act', ACTS)
@pytest.mark.parametrize('net,tile,batch,env,expect', [
    ('myelin2x24', (3, 19, 21), 1, (), 'k_upconv_rows<NCH=3,NTAB=2>'),
    ('semseg_spine', (5, 19, 21), 1, ('SD_UPCONV32_NO_WL',), 'k_upconv_rows<NCH=4,NTAB=2>'),
    ('semseg_spine', (13, 65, 65), 174, (), 'k_upconv_rows<NCH=16,NTAB=8,LDS weights,G=2>'),      # 7 x 9 x 9 x 174 source voxels
    ('semseg_spine', (13, 65, 65), 174, ('SD_UPCONV128_MFMA',), 'k_upconv_mfma'),
    ('semseg_axon', (13, 65, 65), 174, (), 'k_upconv_rows<NCH=24,NTAB=12,LDS weights,G=6>'),
    ('semseg_axon', (13, 65, 65), 174, ('SD_UPCONV192_MFMA',), 'k_upconv_mfma'),
], ids=['3-2', '4-2-no-wl', '16-8-G2', '128-mfma', '24-12-G6', '192-mfma'])
def test_up_convolution_forms(gpu, monkeypatch, net, tile, batch, env, expect, act):
    """The symbols of launch_upconv_t that the small launch sets do not select; odd source extents (the crop is not empty),
    source voxel counts that are no multiple of 128."""
    run_case(gpu, monkeypatch, act, net, tile, batch=batch, env=env, only=r'k_upconv', expect=(expect,))


@pytest.mark.parametrize('act', ACTS)
@pytest.mark.parametrize('net,inp,env,expect', [
    ('semseg_spine', 'u8', (), 'k_conv_first<uint8 input, bf16 MFMA on the exact values>'),
    ('semseg_spine', 'u8', ('SD_NO_FIRST_U8',), 'k_conv_first<uint8 input, f32 MFMA chain>'),
    ('semseg_spine', 'f32', (), 'k_conv_first<float32 input, f32 MFMA chain>'),
    ('cnn3', 'u8', (), 'k_conv_first<uint8 input, f32 MFMA chain>'),
    ('cnn3', 'f32', (), 'k_conv_first<float32 input, f32 MFMA chain>'),
], ids=['planar-u8', 'planar-u8-chain', 'planar-f32', '3x3x3-u8', '3x3x3-f32'])
def test_first_convolution_forms(gpu, monkeypatch, net, inp, env, expect, act):
    run_case(gpu, monkeypatch, act, net, (5, 35, 37), env=env, only=r'k_conv_first', expect=(expect,), inp=inp)


@pytest.mark.parametrize('act', ACTS)
@pytest.mark.parametrize('net,env', [('mivcsj_neg', ()), ('mivcsj_neg', ('SD_NO_GN_FUSE',)), ('mivcsj', ('SD_NO_GN_FUSE',))],
                         ids=['neg', 'neg-nofuse', 'nofuse'])
def test_groupnorm_and_pool_forms(gpu, monkeypatch, net, env, act):
    """GroupNorm composites with statistics from the convolution epilogue and from k_gn_stats, half of the weights negative;
    without SD_NO_GN_FUSE the pooling rides in the apply pass, with it k_maxpool runs (odd extents: ceil mode)."""
    expect = ('k_gn_stats + k_gn_finalize + k_gn_apply', 'k_final_mfma / k_final') + \
             (('k_maxpool',) if env else ('k_gn_finalize + k_gn_apply',))
    run_case(gpu, monkeypatch, act, net, (13, 27, 29), env=env, expect=expect)


def _no_wl_main():
    """Body of the child process of test_up_convolution_forms_without_lds_weights."""
    gpu = torch.device('cuda', 0)
    seen = {}
    with pytest.MonkeyPatch.context() as mp:
        for act in ACTS:
            for net in ('semseg_spine', 'semseg_axon'):
                seen.setdefault(act, []).extend(sorted(run_case(gpu, mp, act, net, (5, 19, 21), only=r'k_upconv')))
    print('NO_WL_RESULT ' + json.dumps(dict(seen=seen, checked=_checked)))


def test_up_convolution_forms_without_lds_weights(gpu):
    """SD_NO_UPCONV_WL is read once per process, so these forms run in a fresh one: 96 -> 48 channels in the plain row kernel,
    128 -> 64 and 192 -> 96 channels in the generic kernel."""
    here = os.path.dirname(os.path.abspath(__file__))
    code = f'import sys; sys.path[:0] = [{here!r}, {os.path.dirname(here)!r}]; import test_gpu_unet_steps as t; t._no_wl_main()'
    cmd = [sys.executable] + (['-s'] if sys.flags.no_user_site else []) + ['-c', code]
    r = subprocess.run(cmd, env=dict(os.environ, SD_NO_UPCONV_WL='1'), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    print('\n'.join(ln for ln in r.stdout.splitlines() if ln.startswith('STEPSTAT')))
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('NO_WL_RESULT ')][-1][len('NO_WL_RESULT '):])
    for act in ACTS:
        ran = set(res['seen'][act])
        assert ran == {'k_upconv_rows<NCH=4,NTAB=2>', 'k_upconv_rows<NCH=6,NTAB=3>', 'k_upconv_mfma'}, ran
    for label, per_act in res['checked'].items():
        for act, r2 in per_act.items():
            rec = _checked.setdefault(label, {}).setdefault(act, dict(n=0, c=-1e9, share=0.0, steps=0.0))
            rec['n'] += r2['n']
            rec['c'], rec['share'], rec['steps'] = max(rec['c'], r2['c']), max(rec['share'], r2['share']), max(rec['steps'], r2['steps'])


def test_every_listed_symbol_was_checked():
    """Runs last in this file: a case that silently fell into another form leaves its symbol unchecked."""
    for label, per_act in sorted(_checked.items()):
        for act, r in sorted(per_act.items()):
            cobs = f'{r["c"]:.2f} of {R.C[act]}' if r['c'] > -1e9 else 'n/a (equality / composite)'
            print(f'STEPTABLE {label} | {act} | ops {r["n"]} | c_obs {cobs} | one-step share {r["share"]:.2e} | max steps {r["steps"]:.1f}')
    missing = [s for s in SYMBOLS for act in ACTS if act not in _checked.get(s, {})]
    assert not missing, f'listed but never checked: {missing}'
    extra = sorted(s for s in _checked if s not in SYMBOLS)
    assert not extra, f'checked but not listed (add them to SYMBOLS): {extra}'
    for label, per_act in _checked.items():
        for act, r in per_act.items():
            assert r['steps'] <= 1.0, f'{label} {act}: an element differs from the rounded reference by {r["steps"]} storage steps'
