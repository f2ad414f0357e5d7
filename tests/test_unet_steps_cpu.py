"""The per-op float64 reference (tests/_unet_step_ref.py) checked without a GPU.

* chained without any rounding it IS the network: compared with the float64 oracle for five networks, which pins the plan
  reading, the fold, the concat order, the crop, ceil-mode pooling and the GroupNorm regions against an independent
  implementation;
* the accumulation constant c_ref recorded in the module is re-measured;
* the rule passes a stand-in for the device (every op in float32 with torch, rounded to storage) and fails it once one
  defect is planted: a dropped (input channel, tap) term, an input shifted by one voxel in the last 16-column block, two
  output channels swapped.
"""
import copy
import functools

import pytest
import torch

from oracle.unet_ref import build_cnn3, build_unet
from syconn_amd.plan import plan_from_model

import _unet_step_ref as R

NETS = ('myelin3x16', 'semseg_spine', 'semseg_axon', 'mivcsj', 'cnn3')
TILES = ((8, 16, 32), (5, 17, 19))
ACTS = ('bf16', 'f16')


@functools.lru_cache(maxsize=None)
def _net(name):
    if name == 'cnn3':
        return build_cnn3(0)
    if name == 'myelin3x16':
        return build_unet('myelin', seed=1, n_blocks=3, start_filts=16)
    return build_unet(name, seed=3)


@functools.lru_cache(maxsize=None)
def _plan(name):
    ops, blob, _ = plan_from_model(_net(name))
    return ops, blob


def _raw(shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, shape, generator=g, dtype=torch.uint8)


@pytest.mark.parametrize('tile', TILES, ids=lambda t: 'x'.join(map(str, t)))
@pytest.mark.parametrize('name', NETS)
def test_chain_equals_float64_oracle(name, tile):
    """Bound 1e-10 of the largest logit.  Both sides are float64 evaluations of the same real function in different
    orders: each of the ~20 layers adds about 1e-16 sqrt(terms) relative, amplified by at most a few hundred through the
    normalisations -- 1e-13 at the worst.  What is NOT float64 on the plan's side is the eps of the normalisations, which an
    OpDesc carries as float32(1e-5): relative 2.5e-8 of a term that is itself 1e-5 of the variance, i.e. 2.5e-13 per layer.
    Any mistake in the plan reading (a swapped concat, a wrong crop or region, a floor-mode pooling) is 1e-3 or more."""
    ops, blob = _plan(name)
    raw = _raw(tile, 7)
    sr = R.StepRef(ops, blob, 'bf16', exact=True)
    _, logits, _ = R.chain(sr, raw)
    with torch.no_grad():
        want = copy.deepcopy(_net(name)).double()((raw.to(torch.float32) / 255.).double()[None, None])[0]
    assert logits.shape == want.shape
    err = float((logits - want).abs().max()) / float(want.abs().max())
    print(f'{name} {tile}: chained float64 steps vs float64 oracle: {err:.2e} of the largest logit')
    assert err <= 1e-10


@functools.lru_cache(maxsize=None)
def _stand_in(name, tile, act):
    """The plan with every op in float32 (torch-CPU) and every stored tensor rounded to storage, and per unit the float64
    reference on the SAME inputs: [(unit, inputs, res32, res64)]."""
    ops, blob = _plan(name)
    sr = R.StepRef(ops, blob, act)
    # (one thread: torch's float32 summation order, and with it c_ref, depends on how the work is split)
    nthreads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        _, _, log = R.chain(sr, _raw(tile, 11), dtype=torch.float32, store=lambda t: R.to_storage(t, act))
    finally:
        torch.set_num_threads(nthreads)
    out = []
    for unit, (x0, x1, region), r32 in log:
        kind, i, _ = unit
        form = 'f32_chain' if (kind == 'conv' and ops[i].src0 == 0) else None
        r64 = sr.compute(unit, x0, x1, form=form, region=region)
        out.append((unit, (x0, x1, region), r32, r64))
    return sr, out


def _stored(sr, r32):
    return r32['ref'].to(torch.float64) if r32['kind'] in ('pool', 'final') else R.to_storage(r32['ref'], sr.act)


@pytest.mark.parametrize('act', ACTS)
def test_accumulation_constant(act):
    """c_ref: the float32 evaluation of every op against the float64 one, in units of 2^-24 S."""
    worst, where = 0.0, None
    for name in NETS:
        for tile in TILES:
            _, units = _stand_in(name, tile, act)
            for unit, _, r32, r64 in units:
                if unit[0] == 'pool':
                    continue
                a, b = (r32['raw'], r64['raw']) if r64['kind'] == 'gn' else (r32['ref'], r64['ref'])
                c = R.c_ratio(a, b, r64['S'])
                if c > worst:
                    worst, where = c, (name, tile, unit)
    print(f'{act}: c_ref = {worst:.3f} at {where}; recorded {R.C_REF[act]}')
    assert worst <= R.C_REF[act]
    assert R.C[act] == 4 * R.C_REF[act]


@pytest.mark.parametrize('act', ACTS)
def test_float32_stand_in_passes_the_rule(act):
    for name in NETS:
        for tile in TILES:
            sr, units = _stand_in(name, tile, act)
            for unit, _, r32, r64 in units:
                nbad, worst, ratio, _ = sr.check(_stored(sr, r32), r64)
                assert nbad == 0, (name, tile, unit, nbad, worst, ratio)


def _defect_units(sr, units):
    """level-0 second convolution (x extent of the tile) and the convolution with the most terms."""
    convs = [k for k, (u, _, _, _) in enumerate(units) if u[0] == 'conv' and sr.ops[u[1]].src0 != 0]

    def terms(k):
        d = sr.ops[units[k][0][1]]
        return (d.cin0 + max(d.cin1, 0)) * d.kz * 9
    return convs[0], max(convs, key=terms)


@pytest.mark.parametrize('act', ACTS)
@pytest.mark.parametrize('name,tile', [('myelin3x16', (5, 17, 19)), ('semseg_spine', (8, 16, 32)), ('mivcsj', (5, 17, 19))])
def test_planted_defects_fail_the_rule(name, tile, act):
    sr, units = _stand_in(name, tile, act)
    first, deep = _defect_units(sr, units)
    for k in sorted({first, deep}):
        unit, (x0, x1, region), r32, r64 = units[k]
        d = sr.ops[unit[1]]
        assert sr.check(_stored(sr, r32), r64)[0] == 0

        # (a) one (input channel, tap) weight zeroed in the stand-in: the first input channel that is alive behind its ReLU
        # at half of the voxels or more (a dead channel's term is zero with or without its weight), a tap off the centre
        xin = x0 if x1 is None else torch.cat((x0[:, :x1.shape[1], :x1.shape[2], :x1.shape[3]], x1), 0)
        ci = next(c for c in range(xin.shape[0]) if float((xin[c] != 0).double().mean()) >= 0.5)

        def drop(w, kz=d.kz // 2, ci=ci):
            w[:, ci, kz, 1, 2] = 0.0
            return w
        bad = sr.compute(unit, x0, x1, dtype=torch.float32, region=region, w_hook=drop)
        nbad, _, ratio, diff = sr.check(_stored(sr, bad), r64)
        pos = r64['ref'] > 0
        over = diff > sr.allowed(r64)
        share = float((over & pos).sum()) / max(int(pos.sum()), 1)
        print(f'{name} {act} unit {unit}: dropped term flags {share:.1%} of the positive outputs (worst {ratio:.1f}x)')
        assert nbad > 0
        assert share >= 0.05, share

        # (c) one output channel swapped with its neighbour
        y = _stored(sr, r32).clone()
        y[[2, 3]] = y[[3, 2]]
        assert sr.check(y, r64)[0] > 0

    # (b) the input shifted by one voxel along x for the last 16-column block only (level 0: W = tile width)
    unit, (x0, x1, region), r32, r64 = units[first]
    W = x0.shape[-1]
    lo = max((W - 1) // 16 * 16, 1)
    xs = x0.clone()
    xs[..., lo:] = x0[..., lo - 1:W - 1]
    bad = sr.compute(unit, xs, x1, dtype=torch.float32, region=region)
    nbad, worst, ratio, diff = sr.check(_stored(sr, bad), r64)
    assert nbad > 0
    if r64['kind'] != 'gn':
        cols = (diff > sr.allowed(r64)).nonzero()[:, -1]
        assert int(cols.min()) >= lo - 1          # only the shifted block (and the column whose halo reaches into it) fails
