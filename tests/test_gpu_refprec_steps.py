"""Every layer form of the two reference-precision U-Net plans -- split-fp16 ('f16x2': sd_split.hip, k_conv_mfma MODE 3, the
split forms of k_conv_first / k_upconv_*) and fp32 FMA ('f32': sd_f32.hip) -- against the float64 reference of that ONE op
(tests/_unet_step_ref.py), the way tests/test_gpu_unet_steps.py does it for the bf16 / f16 plans.

Per case: a `DenseModel` under SD_KEEP_ALL=1 plus the A/B switches the case names, one forward, `op_kernels()` for the symbol
that computed each op; then for every op (or the ops whose label matches the case's filter) the device's own INPUT buffers go
through the float64 reference of that op and the result is compared with the device's OUTPUT buffer, element by element, under
the rule of the reference module: the representation error (f16x2: rep, f32: half a float32 ulp) plus c 2^-24 S plus, for the
split plan, the dropped fourth product D; pooling exact.  A split buffer is read back as the exact float32 sum hi + lo.

A label is the kernel symbol as the launcher notes it; ' +pool' / ' +final' for an op computed in a convolution's epilogue,
'+pool (GroupNorm apply)' for the pooling that rides in `k_gn_apply_pool_split`; the split first convolution (one symbol for
four instantiations) gets its kernel depth and input type appended.  Every case asserts that the form it is named after ran;
a collector gathers the labels that were checked and the last test compares it with SYMBOLS.  The observed c per label is
printed (STEPTABLE; one run is kept in profiles/refprec_steps_table.txt) and not asserted.

Not readable under SD_KEEP_ALL and therefore not here (NOT_COVERED): the first convolution inside its consumer (MODE 4) and the
deferred GroupNorm apply in `k_final_split`; test_gpu_split.py::test_split_fusions_agree_with_the_layer_wise_split_plan pins
them to the forms checked here.
"""
import json
import os
import re
import subprocess
import sys

import pytest
import torch

from syconn_amd.plan import plan_from_model

import _unet_step_ref as R
from test_gpu_unet_steps import SMALL_TILES, _input, _net

pytestmark = pytest.mark.gpu

CONV = 'k_conv_mfma<f16,%s,NT=%d,WAVES=%d,NSLOT=%d,MT=%d,MODE=3>'
FIRST = 'k_conv_first<split-fp16, f32 MFMA chain> [KZ=%d,%s]'
UP = 'k_upconv_rows<split-fp16,NCH=%d,NTAB=%d%s>'
GN_FUSED, GN_FULL = 'k_gn_finalize + k_gn_apply', 'k_gn_stats + k_gn_finalize + k_gn_apply'
K32 = 'k32_conv<%d,%s,%s>'


def _c(k, nt, waves, nslot, mt=2):
    return CONV % (k, nt, waves, nslot, mt)


SYMBOLS = {
    'f16x2': [
        # launch_conv_split_knt, small launch sets: 4 waves, resident weights where they fit 80 KiB, else streamed; the 3x3x3
        # NT = 3 layer with fused GroupNorm statistics in the 8-wave form
        _c('1x3x3', 1, 4, 2), _c('1x3x3', 1, 4, 0), _c('1x3x3', 2, 4, 0), _c('1x3x3', 3, 4, 0),
        _c('3x3x3', 1, 4, 0), _c('3x3x3', 2, 4, 0), _c('3x3x3', 3, 4, 0), _c('3x3x3', 3, 8, 0),
        # ... large launch sets: 8-wave resident, the two four-tile forms and their partners, 8-wave streamed
        _c('1x3x3', 1, 8, 2), _c('1x3x3', 1, 8, 0), _c('3x3x3', 2, 8, 0, 4), _c('3x3x3', 2, 8, 0), _c('1x3x3', 2, 4, 0, 4),
        _c('1x3x3', 2, 8, 0), _c('1x3x3', 3, 8, 0), _c('3x3x3', 1, 8, 0),
        '+pool', '+final', '+pool (GroupNorm apply)',
        # launch_first (one symbol, four instantiations)
        FIRST % (1, 'u8'), FIRST % (1, 'f32'), FIRST % (3, 'u8'), FIRST % (3, 'f32'),
        # launch_upconv, SD_F16X2
        UP % (4, 2, ''), UP % (4, 2, ',LDS weights'), UP % (8, 4, ',LDS weights'), UP % (6, 3, ',LDS weights'),
        UP % (16, 8, ',LDS weights,G=4'), UP % (12, 6, ',LDS weights,G=3'), UP % (12, 6, ''), 'k_upconv_mfma<split-fp16>',
        # launch_pool, launch_final, launch_groupnorm (the split kernels behind the shared GroupNorm symbols)
        'k_maxpool_split', 'k_final_split', GN_FUSED, GN_FULL,
    ],
    'f32': [K32 % (kz, blk, t) for kz in (1, 3) for blk in ('1x16x16', '2x16x8', '4x16x4') for t in ('float',)] +
           [K32 % (kz, blk, 'uint8') for kz in (1, 3) for blk in ('1x16x16', '2x16x8', '4x16x4')] +
           ['k32_upconv<1>', 'k32_upconv<2>', 'k32_pool', 'k32_gn_stats + k32_gn_apply', 'k32_final'],
}
NOT_COVERED = {
    'k_conv_mfma<f16,1x3x3,NT=1,WAVES=8,NSLOT=4,MT=2,MODE=4>':
        'the first convolution inside its consumer: its output is not stored, so the consumer has no readable input under '
        'SD_KEEP_ALL; pinned by test_split_fusions_agree_with_the_layer_wise_split_plan and the 128^3 label tests',
    'k_gn_stats + k_gn_finalize / k_gn_finalize (deferred apply in k_final_split)':
        'SD_KEEP_ALL switches the deferral off (defer_groupnorms, sd_plan.cpp); pinned by the same test',
    'k_conv_mfma<f16,...,NSLOT=2,...> with NT >= 2 or 3x3x3':
        'the resident-weight rules (80 / 96 KiB of LDS for three virtual chunks per input chunk) admit no such layer of the path: '
        'the smallest, 16 -> 16 channels 3x3x3, needs 81 KiB of weights (it runs as NSLOT=0, which is checked)',
}

_checked = {}        # label -> {act: dict(n, worst c_obs, worst ratio)}
_refs = {}


def _ref(name, act):
    if (name, act) not in _refs:
        ops, blob, _ = plan_from_model(_net(name))
        _refs[(name, act)] = R.StepRef(ops, blob, act)
    return _refs[(name, act)]


def _block_pos(label, idx, shape, d):
    """position of output element (c, z, y, x) inside the block of the form that computed it."""
    c, z, y, x = idx
    m = re.match(r'k_conv_mfma<f16,(\d)x3x3,NT=(\d+),WAVES=(\d+),NSLOT=(-?\d+),MT=(\d+)', label)
    if m:
        kz, nt, waves, _, mt = (int(v) for v in m.groups())
        bz, by = ((waves // 4) * mt, 8) if kz == 3 else (1, waves * 2 * mt)
        return (f'block {bz}x{by}x16 at (z,y,x) = ({z % bz},{y % by},{x % 16}), channel tile {c // 32} of {nt} per workgroup, '
                f'chunk {c // 16}')
    m = re.match(r'k32_conv<(\d),(\d+)x(\d+)x(\d+),', label)
    if m:
        _, tz, ty, tx = (int(v) for v in m.groups())
        return f'block {tz}x{ty}x{4 * tx} at (z,y,x) = ({z % tz},{y % ty},{x % (4 * tx)}), x-quad lane {x % 4}, channel block {c // 16}'
    if label.startswith('k_conv_first'):
        bz, by = (2, 8) if d.kz == 3 else (1, 16)
        return f'block {bz}x{by}x16 at ({z % bz},{y % by},{x % 16})'
    if label.startswith('k_upconv') or label.startswith('k32_upconv'):
        src = ((z // d.kz) * (shape[2] // 2) + y // 2) * (shape[3] // 2) + x // 2
        per = 128 if 'rows' in label else 256
        return f'tap ({z % d.kz},{y % 2},{x % 2}), source voxel {src % per} of its {per}-voxel workgroup'
    return f'voxel {(z * shape[2] + y) * shape[3] + x} % 256 = {((z * shape[2] + y) * shape[3] + x) % 256}'


def run_case(gpu, monkeypatch, act, net, tile, batch=1, env=(), only=None, expect=(), inp='u8', seed=0):
    """One model, one forward, every op (or those matching `only`) against its float64 reference.  Returns the labels checked."""
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
    seen, failures, bufs = set(), [], {}

    def buf(b):
        if b not in bufs:
            bufs[b] = dm.read_buffer(b).cpu().to(torch.float64)
        return bufs[b]

    for unit in sr.units():
        kind, i, g = unit
        d = sr.ops[i]
        e, sym = ks[i]
        assert e >= 0 and sym, (i, ks[i])
        label = sym
        if kind == 'conv' and d.src0 == 0 and act == 'f16x2':
            label = f'{sym} [KZ={d.kz},{inp}]'
        labels = [label]
        if kind == 'pool' and e != i:
            labels = ['+pool (GroupNorm apply)' if sr.ops[e].kind == R.SD_OP_GROUPNORM else '+pool', label]
        if kind == 'final' and e != i:
            labels = ['+final', label]
        if g >= 0:
            labels.append(ks[g][1])
        if only is not None and not any(re.search(only, s) for s in labels):
            continue
        form = None
        if kind == 'conv' and d.src0 == 0:
            form, x0 = 'f32_chain', xin[0]
        else:
            x0 = buf(d.src0)
        if kind == 'final':
            form = 'f32' if (act == 'f32' or e == i) else 'hilo'
        x1 = buf(d.src1) if (kind == 'conv' and d.src1 >= 0) else None
        region = tuple(buf(sr.ops[g].src1).shape[1:]) if (g >= 0 and sr.ops[g].src1 >= 0) else None
        res = sr.compute(unit, x0, x1, form=form, region=region)
        dev = logits.to(torch.float64) if kind == 'final' else buf(d.dst)
        if region is not None:
            dev = dev[:, :region[0], :region[1], :region[2]]
        nbad, worst, ratio, diff = sr.check(dev, res)
        seen.update(labels)
        cobs = -1e9
        if res['kind'] not in ('pool', 'gn'):
            ref = res['ref']
            half = (R.ulp_f32(ref.abs()) if kind == 'final' else R.ulp_s(ref.abs(), act)) / 2
            dropped = res['D'] if res['D'] is not None else 0.0
            cobs = float(((diff - half - dropped) / (2.0 ** -24 * res['S'].clamp_min(1e-300))).max())
        for s in labels[:1] if labels[0].startswith('+') else labels:
            rec = _checked.setdefault(s, {}).setdefault(act, dict(n=0, c=-1e9, ratio=0.0))
            rec['n'] += 1
            rec['c'], rec['ratio'] = max(rec['c'], cobs), max(rec['ratio'], ratio)
        print(f'STEPSTAT {act} {net} {tile}x{batch} op {i} {" | ".join(labels)} ratio {ratio:.3f} c_obs {cobs:.2f}')
        if nbad:
            idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(worst), dev.shape))
            failures.append(f'op {i} [{" | ".join(labels)}]: {nbad} of {dev.numel()} elements over the rule; worst at channel '
                            f'{idx[0]}, (z,y,x) = {idx[1:]} of {tuple(dev.shape[1:])}: {_block_pos(label, idx, dev.shape, d)}; '
                            f'dev {float(dev[idx]):.9g} ref {float(res["ref"][idx]):.9g}, {ratio:.1f} x the allowed difference')
    assert not failures, f'{net} {act} tile {tile} x {batch} {sorted(env)}:\n' + '\n'.join(failures)
    for s in expect:
        assert s in seen, f'{net} {tile} x {batch} {sorted(env)}: form {s} did not run; ran {sorted(seen)}'
    return seen


# ---- f16x2 ---------------------------------------------------------------------------------------------------------------
SPLIT_SMALL_EXPECT = {      # the forms every tile of these launch sets selects (verified on the device, not by arithmetic)
    'myelin3x16': (_c('1x3x3', 1, 4, 2), _c('1x3x3', 2, 4, 0), _c('3x3x3', 1, 4, 0), '+pool', '+final', FIRST % (1, 'u8'),
                   UP % (4, 2, ',LDS weights'), 'k_upconv_mfma<split-fp16>'),
    'semseg_spine': (_c('1x3x3', 1, 4, 2), _c('1x3x3', 1, 4, 0), _c('1x3x3', 2, 4, 0), _c('3x3x3', 2, 4, 0), '+pool', '+final',
                     FIRST % (1, 'u8'), UP % (4, 2, ',LDS weights'), UP % (8, 4, ',LDS weights'), 'k_upconv_mfma<split-fp16>'),
    'syntype': (_c('1x3x3', 1, 4, 2), _c('1x3x3', 1, 4, 0), _c('3x3x3', 2, 4, 0), '+pool', '+final', FIRST % (1, 'u8'),
                UP % (4, 2, ',LDS weights'), 'k_upconv_mfma<split-fp16>'),
    'semseg_axon': (_c('1x3x3', 2, 4, 0), _c('1x3x3', 3, 4, 0), _c('3x3x3', 3, 4, 0), '+pool', '+final', FIRST % (1, 'u8'),
                    UP % (6, 3, ',LDS weights'), UP % (12, 6, ',LDS weights,G=3'), 'k_upconv_mfma<split-fp16>'),
    'mivcsj': (_c('1x3x3', 2, 4, 0), _c('1x3x3', 3, 4, 0), _c('3x3x3', 3, 8, 0), 'k_final_split', GN_FUSED, GN_FULL,
               '+pool (GroupNorm apply)', FIRST % (1, 'u8'), UP % (6, 3, ',LDS weights'), UP % (12, 6, ',LDS weights,G=3'),
               'k_upconv_mfma<split-fp16>'),
    'cnn3': (_c('3x3x3', 1, 4, 0), FIRST % (3, 'u8'), 'k_final_split'),
}


@pytest.mark.parametrize('tile', SMALL_TILES, ids=lambda t: 'x'.join(map(str, t)))
@pytest.mark.parametrize('net', list(SPLIT_SMALL_EXPECT))
def test_split_all_ops_small_launch_sets(gpu, monkeypatch, net, tile):
    """Every op of six networks on tiles where every voxel is a border voxel, D = 1, W < 16, odd extents through ceil-mode
    pooling and crop, and extents one above / below a multiple of the block extents: the 4-wave resident and streamed forms,
    the fused pooling, both final-layer forms, the GroupNorm composites with fused and separate statistics."""
    run_case(gpu, monkeypatch, 'f16x2', net, tile, expect=SPLIT_SMALL_EXPECT[net])


LARGE_CASES = [
    # (vox / 512) NB >= 256 and the weights of three virtual chunks per input chunk within 96 KiB: level 0 of the 32-filter nets
    ('semseg_spine', (8, 129, 129), 1, (), r'WAVES=8,NSLOT=2', _c('1x3x3', 1, 8, 2)),
    # ... past 96 KiB (the 64 -> 32 merge convolution of the same launch set): 8-wave streamed
    ('semseg_spine', (8, 129, 129), 1, (), r'1x3x3,NT=1,WAVES=8,NSLOT=0', _c('1x3x3', 1, 8, 0)),
    ('myelin3x16', (9, 65, 49), 20, (), r'3x3x3,NT=1,WAVES=8,NSLOT=0', _c('3x3x3', 1, 8, 0)),
    # 64-channel 3x3x3 layers of level 1 at 13 x 73 x 73 x 4 tiles: (vox / 1024) NB >= 256 and the z rule; the MT = 2 partner
    # through the stricter z rule of SD_MT4_D_RULE (13 is neither a multiple of 8 nor >= 96)
    ('semseg_spine', (13, 145, 145), 4, (), r'3x3x3,NT=2,WAVES=8', _c('3x3x3', 2, 8, 0, 4)),
    ('semseg_spine', (13, 145, 145), 4, ('SD_MT4_D_RULE',), r'3x3x3,NT=2,WAVES=8', _c('3x3x3', 2, 8, 0)),
    # 128-channel planar layers of level 2 at 30 x 33 x 31 x 9 tiles: (vox / 512) NB >= 1024
    ('semseg_spine', (60, 130, 122), 9, (), r'1x3x3,NT=2,WAVES=[48],NSLOT=0', _c('1x3x3', 2, 4, 0, 4)),
    ('semseg_spine', (60, 130, 122), 9, ('SD_NO_PLANAR4',), r'1x3x3,NT=2,WAVES=[48],NSLOT=0', _c('1x3x3', 2, 8, 0)),
    # 192-channel planar layers of semseg_axon's level 2 at 15 x 33 x 31 x 5 tiles: 4 waves unless SD_PLANAR_NT3_BIG
    ('semseg_axon', (30, 130, 122), 5, (), r'1x3x3,NT=3,WAVES=4', _c('1x3x3', 3, 4, 0)),
    ('semseg_axon', (30, 130, 122), 5, ('SD_PLANAR_NT3_BIG',), r'1x3x3,NT=3,WAVES=8', _c('1x3x3', 3, 8, 0)),
    # 3x3x3 NT = 3 with fused GroupNorm statistics at a large launch set (mivcsj level 1, 9 x 33 x 33 x 16 tiles)
    ('mivcsj', (9, 65, 65), 16, (), r'3x3x3,NT=3,WAVES=8', _c('3x3x3', 3, 8, 0)),
]


@pytest.mark.parametrize('net,tile,batch,env,only,expect', LARGE_CASES, ids=['wres8', 'stream8-planar', 'stream8-3x3x3', 'MT4', 'MT2-partner', 'planar4', 'SD_NO_PLANAR4', 'NT3-4wave', 'NT3-big',
        'NT3-gn-sums'])
def test_split_large_launch_set_forms(gpu, monkeypatch, net, tile, batch, env, only, expect):
    """The remaining branches of launch_conv_split_knt at the smallest launch sets that select them; only the ops of the named
    form are checked."""
    run_case(gpu, monkeypatch, 'f16x2', net, tile, batch=batch, env=env, only=only, expect=(expect,))


@pytest.mark.parametrize('net,inp,kz', [('semseg_spine', 'u8', 1), ('semseg_spine', 'f32', 1), ('cnn3', 'u8', 3), ('cnn3', 'f32', 3)],
                         ids=['planar-u8', 'planar-f32', '3x3x3-u8', '3x3x3-f32'])
def test_split_first_convolution_forms(gpu, monkeypatch, net, inp, kz):
    run_case(gpu, monkeypatch, 'f16x2', net, (5, 35, 37), only=r'k_conv_first', expect=(FIRST % (kz, inp),), inp=inp)


UPCONV_CASES = [
    ('semseg_spine', (5, 19, 21), 1, ('SD_SPLIT_ROWS32_NO_WL',), UP % (4, 2, '')),
    ('semseg_spine', (13, 65, 65), 174, (), UP % (16, 8, ',LDS weights,G=4')),      # 7 x 9 x 9 x 174 source voxels >= 98304
    ('semseg_spine', (13, 65, 65), 174, ('SD_SPLIT_UPCONV128_MFMA',), 'k_upconv_mfma<split-fp16>'),
    ('semseg_axon', (5, 19, 21), 1, ('SD_SPLIT_ROWS96_L2',), UP % (12, 6, '')),
    ('semseg_axon', (5, 19, 21), 1, ('SD_SPLIT_NO_ROWS96',), 'k_upconv_mfma<split-fp16>'),
]


@pytest.mark.parametrize('net,tile,batch,env,expect', UPCONV_CASES, ids=['4-2-no-wl', '16-8-G4', '128-mfma', '12-6-L2', '96-mfma'])
def test_split_up_convolution_forms(gpu, monkeypatch, net, tile, batch, env, expect):
    """The shapes launch_upconv distinguishes for the split plan that the small launch sets do not select; odd source extents
    (the crop is not empty), source voxel counts that are no multiple of 128."""
    run_case(gpu, monkeypatch, 'f16x2', net, tile, batch=batch, env=env, only=r'k_upconv', expect=(expect,))


@pytest.mark.parametrize('net,env', [('mivcsj_neg', ()), ('mivcsj_neg', ('SD_NO_GN_FUSE',)), ('mivcsj', ('SD_NO_GN_FUSE',)),
                                     ('mivcsj', ('SD_NO_FUSE',)), ('semseg_spine', ('SD_NO_FUSE',))],
                         ids=['neg', 'neg-nofuse', 'nofuse', 'gn-layerwise', 'bn-layerwise'])
def test_split_groupnorm_pool_and_final_forms(gpu, monkeypatch, net, env):
    """GroupNorm composites with statistics from the convolution epilogue and from k_gn_stats_split, half of the weights
    negative; without SD_NO_GN_FUSE the pooling rides in the apply pass (k_gn_apply_pool_split, odd extents: ceil mode), with
    it or with SD_NO_FUSE k_maxpool_split runs; SD_NO_FUSE also makes k_final_split the final layer of a BatchNorm net."""
    expect = [GN_FULL, 'k_final_split']
    if net == 'semseg_spine':
        expect = ['k_final_split', 'k_maxpool_split']
    elif env:
        expect.append('k_maxpool_split')
    else:
        expect += [GN_FUSED, '+pool (GroupNorm apply)']
    run_case(gpu, monkeypatch, 'f16x2', net, (13, 27, 29), env=env, expect=expect)


def _no_rows_main():
    """Body of the child process of test_split_up_convolution_forms_without_the_row_kernels."""
    gpu = torch.device('cuda', 0)
    seen = []
    with pytest.MonkeyPatch.context() as mp:
        for net in ('semseg_spine', 'semseg_axon'):
            seen.extend(sorted(run_case(gpu, mp, 'f16x2', net, (5, 19, 21), only=r'k_upconv')))
    print('NO_ROWS_RESULT ' + json.dumps(dict(seen=seen, checked=_checked)))


def test_split_up_convolution_forms_without_the_row_kernels(gpu):
    """SD_SPLIT_NO_ROWS is read once per process, so the generic kernel at the row kernels' shapes (64 -> 32, 128 -> 64, 96 -> 48,
    192 -> 96 channels) runs in a fresh one."""
    here = os.path.dirname(os.path.abspath(__file__))
    code = f'import sys; sys.path[:0] = [{here!r}, {os.path.dirname(here)!r}]; import test_gpu_refprec_steps as t; t._no_rows_main()'
    cmd = [sys.executable] + (['-s'] if sys.flags.no_user_site else []) + ['-c', code]
    r = subprocess.run(cmd, env=dict(os.environ, SD_SPLIT_NO_ROWS='1'), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    print('\n'.join(ln for ln in r.stdout.splitlines() if ln.startswith('STEPSTAT')))
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('NO_ROWS_RESULT ')][-1][len('NO_ROWS_RESULT '):])
    assert set(res['seen']) == {'k_upconv_mfma<split-fp16>'}, res['seen']
    for label, per_act in res['checked'].items():
        for act, r2 in per_act.items():
            rec = _checked.setdefault(label, {}).setdefault(act, dict(n=0, c=-1e9, ratio=0.0))
            rec['n'] += r2['n']
            rec['c'], rec['ratio'] = max(rec['c'], r2['c']), max(rec['ratio'], r2['ratio'])


# ---- f32 -----------------------------------------------------------------------------------------------------------------
F32_TILES = SMALL_TILES + [(6, 70, 130)]
F32_LEVEL0_CLASS = {      # block shape of the level-0 layers on the tile: W > 40, 21 ... 40, <= 20 (verified on the device)
    (1, 1, 1): '4x16x4', (2, 3, 5): '4x16x4', (3, 16, 2): '4x16x4', (1, 40, 33): '2x16x8', (5, 17, 50): '1x16x16',
    (13, 27, 29): '2x16x8', (9, 35, 37): '2x16x8', (6, 70, 130): '1x16x16',
}


@pytest.mark.parametrize('tile', F32_TILES, ids=lambda t: 'x'.join(map(str, t)))
@pytest.mark.parametrize('net', list(SPLIT_SMALL_EXPECT))
def test_f32_all_ops(gpu, monkeypatch, net, tile):
    """Every op of the six networks in the fp32 FMA plan.  Between them the tiles put every layer kind into the three width
    classes (W > 40, 21 ... 40, <= 20) with 63 / 64 / 65 (130, 65), 31 / 32 / 33 and 15 / 16 / 17 columns at the block edges
    and ragged TZ = 2 / 4 blocks in depth; the deeper levels' classes are what the collector sees."""
    cls = F32_LEVEL0_CLASS[tile]
    if net == 'cnn3':
        expect = [K32 % (3, cls, 'uint8'), K32 % (3, cls, 'float'), 'k32_final']
    else:
        expect = [K32 % (1, cls, 'uint8'), K32 % (1, cls, 'float'), 'k32_pool', 'k32_upconv<1>', 'k32_upconv<2>', 'k32_final']
        if net == 'mivcsj':
            expect.append('k32_gn_stats + k32_gn_apply')
    run_case(gpu, monkeypatch, 'f32', net, tile, expect=expect)


@pytest.mark.parametrize('net,inp,batch', [('semseg_spine', 'f32', 1), ('cnn3', 'f32', 1), ('semseg_axon', 'u8', 3), ('mivcsj', 'f32', 3)],
                         ids=['planar-f32-input', '3x3x3-f32-input', 'batch3', 'groupnorm-batch3-f32-input'])
def test_f32_inputs_and_batch(gpu, monkeypatch, net, inp, batch):
    """float32 input (the first convolution is then the `float` instantiation) and a batch of 3 (tile 0 is read back)."""
    kz = 3 if net == 'cnn3' else 1
    run_case(gpu, monkeypatch, 'f32', net, (5, 17, 50), batch=batch, inp=inp,
             expect=(K32 % (kz, '1x16x16', 'float' if inp == 'f32' else 'uint8'), 'k32_final'))


def test_every_listed_symbol_was_checked():
    """Runs last in this file: a case that silently fell into another form leaves its symbol unchecked."""
    for label, per_act in sorted(_checked.items()):
        for act, r in sorted(per_act.items()):
            cobs = f'{r["c"]:.2f} of {R.C[act]}' if r['c'] > -1e9 else 'n/a (equality / composite)'
            print(f'STEPTABLE {label} | {act} | ops {r["n"]} | c_obs {cobs} | worst |dev - ref| / allowed {r["ratio"]:.3f}')
    for act, listed in SYMBOLS.items():
        missing = [s for s in listed if act not in _checked.get(s, {})]
        assert not missing, f'{act}: listed but never checked: {missing}'
        extra = sorted(s for s, per_act in _checked.items() if act in per_act and s not in listed)
        assert not extra, f'{act}: checked but not listed (add them to SYMBOLS): {extra}'
