"""The host-only plan builder (syconn_amd/csrc/sd_plan.cpp) through tools/plan_dump, without a GPU: every reason for which
build_plan refuses a plan, and the workspace layout's invariants."""
import functools
import os
import struct
import subprocess

import numpy as np
import pytest

from oracle.unet_ref import build_cnn3, build_unet
from syconn_amd import _lib as L
from syconn_amd.plan import _desc, plan_from_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONV, POOL, UPCONV, GROUPNORM, FINAL = 1, 2, 3, 4, 5
SD_ERR_INVALID = -1
DTYPES = ('bf16', 'f16', 'f16x2')


@pytest.fixture(scope='module')
def plan_dump(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('plan_dump') / 'plan_dump')
    hipcc = '/opt/rocm/bin/hipcc'
    assert os.path.isfile(hipcc), 'hipcc is needed to build tools/plan_dump.cpp'
    subprocess.run([hipcc, '-O2', '-std=c++17', '-pthread', os.path.join(ROOT, 'syconn_amd', 'csrc', 'sd_plan.cpp'),
                    os.path.join(ROOT, 'tools', 'plan_dump.cpp'), '-o', exe], check=True, timeout=600)
    return exe


def _write_plan(path, ops, blob):
    arr = (L.OpDesc * len(ops))(*ops)
    blob = np.ascontiguousarray(blob, np.float32)
    with open(path, 'wb') as f:
        f.write(b'SDPLAN1\0' + struct.pack('<iq', len(ops), blob.size) + bytes(arr) + blob.tobytes())


def _run(exe, path, *args, env=()):
    r = subprocess.run([exe, str(path), *args], env=dict(os.environ, **{k: '1' for k in env}), capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr
    return r.stdout.splitlines()


# ---- refused plans ----------------------------------------------------------------------------------------------------------------
N_FLOATS = 32768      # all zeros; the offsets below lie inside unless a case moves one out


def _conv(src0, dst, cin0, cout, w_off, b_off, kz=1, **kw):
    return _desc(kind=CONV, src0=src0, dst=dst, cin0=cin0, cout=cout, kz=kz, ky=3, kx=3, relu=1, w_off=w_off, b_off=b_off, **kw)


def _base():
    """first conv 1 -> 8 (buffer 1), conv 8 -> 8 (buffer 2), final 8 -> 2: a valid plan."""
    return [_conv(0, 1, 1, 8, 0, 72), _conv(1, 2, 8, 8, 80, 656), _desc(kind=FINAL, src0=2, cin0=8, cout=2, w_off=664, b_off=680)]


def _with(i, **kw):
    ops = _base()
    for k, v in kw.items():
        setattr(ops[i], k, v)
    return ops


def _insert(i, op):
    ops = _base()
    ops.insert(i, op)
    return ops


_BN = dict(norm=1, gamma_off=700, beta_off=710, mean_off=720, var_off=730)
_UP = dict(kind=UPCONV, src0=2, dst=3, cin0=8, cout=8, kz=1, ky=2, kx=2, w_off=1000, b_off=1300)
_GN = dict(kind=GROUPNORM, src0=2, dst=2, groups=4, gamma_off=700, beta_off=710)
_OUT = N_FLOATS - 3      # an offset whose array ends past the blob

REFUSED = {
    'kernel size ky': (_with(1, ky=5), 'conv: only 3x3x3 and 1x3x3 kernels'),
    'kernel size kz': (_with(1, kz=2), 'conv: only 3x3x3 and 1x3x3 kernels'),
    'conv dst 0': (_with(1, dst=0), 'conv: bad buffer ids'),
    'conv src0 < 0': (_with(1, src0=-1), 'conv: bad buffer ids'),
    'conv cout 0': (_with(1, cout=0), 'conv: bad buffer ids'),
    'first conv, two channels': (_with(0, cin0=2), 'first conv must have exactly one input channel'),
    'first conv, two inputs': (_with(0, src1=0, cin1=1), 'first conv must have exactly one input channel'),
    'cin0 mismatch': (_with(1, cin0=7), 'conv: cin0 does not match producer of src0'),
    'cin1 mismatch': (_with(1, src1=1, cin1=7), 'conv: cin1 does not match producer of src1'),
    'conv w_off': (_with(1, w_off=_OUT), 'conv: weight offsets'),
    'conv w_off < 0': (_with(1, w_off=-1), 'conv: weight offsets'),
    'conv b_off': (_with(1, b_off=_OUT), 'conv: weight offsets'),
    'conv gamma_off': (_with(1, **dict(_BN, gamma_off=_OUT)), 'conv: norm offsets'),
    'conv beta_off': (_with(1, **dict(_BN, beta_off=_OUT)), 'conv: norm offsets'),
    'conv mean_off': (_with(1, **dict(_BN, mean_off=_OUT)), 'conv: norm offsets'),
    'conv var_off': (_with(1, **dict(_BN, var_off=-1)), 'conv: norm offsets'),
    'pool kz': (_insert(2, _desc(kind=POOL, src0=2, dst=3, kz=3)), 'pool: bad arguments'),
    'pool src0': (_insert(2, _desc(kind=POOL, src0=0, dst=3, kz=1)), 'pool: bad arguments'),
    'pool dst': (_insert(2, _desc(kind=POOL, src0=2, dst=0, kz=1)), 'pool: bad arguments'),
    'upconv kz': (_insert(2, _desc(**dict(_UP, kz=3))), 'upconv: bad arguments'),
    'upconv src0': (_insert(2, _desc(**dict(_UP, src0=0))), 'upconv: bad arguments'),
    'upconv cin0': (_insert(2, _desc(**dict(_UP, cin0=16))), 'upconv: cin0 does not match producer'),
    'upconv w_off': (_insert(2, _desc(**dict(_UP, w_off=_OUT))), 'upconv: weight offsets'),
    'upconv b_off': (_insert(2, _desc(**dict(_UP, b_off=_OUT))), 'upconv: weight offsets'),
    'upconv mean_off': (_insert(2, _desc(**dict(_UP, **dict(_BN, mean_off=_OUT)))), 'upconv: norm offsets'),
    'groupnorm groups 0': (_insert(2, _desc(**dict(_GN, groups=0))), 'groupnorm: bad arguments'),
    'groupnorm src0': (_insert(2, _desc(**dict(_GN, src0=0))), 'groupnorm: bad arguments'),
    'groupnorm groups': (_insert(2, _desc(**dict(_GN, groups=3))), 'groupnorm: channels not divisible by groups'),
    # 2576 padded channels: 2 * 2576 doubles of sums do not fit in front of the scale / shift part of the 64 KiB scratch
    'groupnorm channels': ([_conv(0, 1, 1, 2576, 0, 23184), _desc(**dict(_GN, src0=1, dst=1, groups=8, gamma_off=0, beta_off=0)),
                            _desc(kind=FINAL, src0=1, cin0=2576, cout=2, w_off=0, b_off=0)], 'groupnorm: too many channels'),
    'groupnorm gamma_off': (_insert(2, _desc(**dict(_GN, gamma_off=_OUT))), 'groupnorm: offsets'),
    'groupnorm beta_off': (_insert(2, _desc(**dict(_GN, beta_off=-1))), 'groupnorm: offsets'),
    'final 0 classes': (_with(2, cout=0), 'final conv: 1..8 output classes supported'),
    'final 9 classes': (_with(2, cout=9), 'final conv: 1..8 output classes supported'),
    'final cin0': (_with(2, cin0=4), 'final: cin0 does not match producer'),
    'final w_off': (_with(2, w_off=_OUT), 'final: weight offsets'),
    'final b_off': (_with(2, b_off=N_FLOATS - 1), 'final: weight offsets'),
    'unknown kind': (_with(1, kind=9), 'unknown op kind'),
    'no final': (_base()[:2], 'the plan must end with SD_OP_FINAL'),
    'final not last': (_base() + [_conv(2, 3, 8, 8, 80, 656)], 'the plan must end with SD_OP_FINAL'),
}


def test_base_plan_is_valid(plan_dump, tmp_path):
    """The plan the refused ones are one change away from builds, with and without BatchNorm, up-convolution and GroupNorm."""
    for k, ops in enumerate([_base(), _with(1, **_BN), _insert(2, _desc(kind=POOL, src0=2, dst=3, kz=1))[:3] +
                             [_desc(**dict(_UP, src0=3, dst=4, **_BN)), _desc(**dict(_GN, src0=4, dst=4)),
                              _desc(kind=FINAL, src0=4, cin0=8, cout=8, w_off=664, b_off=680)]]):
        _write_plan(tmp_path / f'p{k}.bin', ops, np.zeros(N_FLOATS, np.float32))
        lines = _run(plan_dump, tmp_path / f'p{k}.bin')
        assert [ln for ln in lines if ln.startswith('dtype')] == [f'dtype {t} rc 0' for t in DTYPES]


@pytest.mark.parametrize('case', list(REFUSED))
def test_refused_plan(plan_dump, tmp_path, case):
    """One malformed plan per reason: SD_ERR_INVALID and the message, for every storage type, and nothing else printed."""
    ops, msg = REFUSED[case]
    _write_plan(tmp_path / 'p.bin', ops, np.zeros(N_FLOATS, np.float32))
    assert _run(plan_dump, tmp_path / 'p.bin', '--tile', '8,16,16') == [f'dtype {t} rc {SD_ERR_INVALID} error: {msg}' for t in DTYPES]


# ---- workspace layout -------------------------------------------------------------------------------------------------------------
TILES = ((13, 27, 29), (24, 40, 48))


@functools.lru_cache(maxsize=None)
def _layouts(exe, tmp, net, env):
    """{(dtype, tile): dict(ws_base, workspace, life=[(first, last, off, bytes)])} of one net, from one plan_dump run."""
    model = build_cnn3(0) if net == 'cnn3' else build_unet(net, seed=3)
    ops, blob, _ = plan_from_model(model)
    path = os.path.join(tmp, net + '.bin')
    if not os.path.isfile(path):
        _write_plan(path, ops, blob)
    args = ['--lifetimes', '--dtypes', 'bf16,f16x2']
    for t in TILES:
        args += ['--tile', '%d,%d,%d' % t]
    out, dtype, cur = {}, None, None
    for ln in _run(exe, path, *args, env=env):
        w = ln.split()
        if w[0] == 'dtype':
            assert w[3] == '0', ln
            dtype = w[1]
        elif w[0] == 'nbuf':
            ws_base = int(w[3])
        elif w[0] == 'tile':
            cur = out[(dtype, tuple(int(x) for x in w[1:4]))] = dict(ws_base=ws_base, life=[])
        elif w[0] == 'use_dec0':
            cur['workspace'] = int(w[3])
        elif w[0] == 'life':
            cur['life'].append(tuple(int(w[k]) for k in (3, 5, 7, 9)))
    assert len(out) == 2 * len(TILES)
    return out


@pytest.fixture(scope='module')
def plan_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp('plans'))


@pytest.mark.parametrize('net', ['semseg_spine', 'mivcsj', 'cnn3'])
def test_workspace_layout(plan_dump, plan_dir, net):
    """No two buffers alive at the same op overlap, every buffer lies behind ws_base, and the workspace is the highest end rounded
    to 256 bytes."""
    for key, lay in _layouts(plan_dump, plan_dir, net, ()).items():
        used = [x for x in lay['life'] if x[1] >= 0 and x[3] > 0]
        assert used, key
        for k, (f0, l0, o0, n0) in enumerate(used):
            assert o0 >= lay['ws_base'] and o0 % 256 == 0, (key, k)
            # (first > last: read by an op that runs inside another launch and never written -- a range, but never alive)
            for f1, l1, o1, n1 in used[:k]:
                if f0 <= l1 and f1 <= l0 and f0 <= l0 and f1 <= l1:
                    assert o0 + n0 <= o1 or o1 + n1 <= o0, (key, (f0, l0, o0, n0), (f1, l1, o1, n1))
        top = max(o + n for _, _, o, n in used)
        assert lay['workspace'] == (top + 255) // 256 * 256, key


@pytest.mark.parametrize('net', ['semseg_spine', 'mivcsj', 'cnn3'])
@pytest.mark.parametrize('env', ['SD_KEEP_ALL', 'SD_NO_FUSE', 'SD_NO_WS_REUSE'])
def test_workspace_without_reuse(plan_dump, plan_dir, net, env):
    """With reuse off every buffer has its own range: the total is ws_base plus the sum of the buffer sizes."""
    for key, lay in _layouts(plan_dump, plan_dir, net, (env,)).items():
        assert lay['workspace'] == lay['ws_base'] + sum(x[3] for x in lay['life']), key
        ranges = sorted((o, o + n) for _, _, o, n in lay['life'] if n)
        assert ranges[0][0] >= lay['ws_base'] and all(a[1] <= b[0] for a, b in zip(ranges, ranges[1:])), key
