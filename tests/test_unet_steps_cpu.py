"""The per-op float64 reference (tests/_unet_step_ref.py) checked without a GPU.

* chained without any rounding it IS the network: compared with the float64 oracle for five networks, which pins the plan
  reading, the fold, the concat order, the crop, ceil-mode pooling and the GroupNorm regions against an independent
  implementation;
* the accumulation constant c_ref recorded in the module is re-measured;
* the rule passes a stand-in for the device (every op in float32 with torch, rounded to storage) and fails it once one
  defect is planted: a dropped (input channel, tap) term, an input shifted by one voxel in the last 16-column block, two
  output channels swapped;
* the same for the two reference-precision representations 'f16x2' and 'f32': the split representation itself (exact float32
  sum, |v - (hi + lo)| <= rep(v), attained), a stand-in that emulates the split plan from its parts (three products in one
  float32 accumulation), and the defects a split or an fp32 kernel can have: a dropped low-order pass, a low part not read at
  one tap, hi / lo planes of neighbouring chunks paired, a tap missing on one face, a low part not stored, a tap missing at
  one border voxel, a channel of the second concatenation source skipped.
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
ACTS = ('bf16', 'f16', 'f16x2', 'f32')
# final-layer forms of a representation: the chain runs the first, the others are computed on the same input as well
FINAL_FORMS = {'bf16': (None,), 'f16': (None,), 'f16x2': ('hilo', 'f32'), 'f32': ('f32',)}


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
        _, _, log = R.chain(sr, _raw(tile, 11), dtype=torch.float32, store=lambda t: R.to_storage(t, act),
                            final_form=FINAL_FORMS[act][0])
        unit, (x0, x1, region), _ = log[-1]
        for form in FINAL_FORMS[act][1:]:
            log.append((unit, (x0, x1, region), sr.compute(unit, x0, form=form, dtype=torch.float32)))
    finally:
        torch.set_num_threads(nthreads)
    out = []
    finals = iter(FINAL_FORMS[act])
    for unit, (x0, x1, region), r32 in log:
        kind, i, _ = unit
        form = 'f32_chain' if (kind == 'conv' and ops[i].src0 == 0) else (next(finals) if kind == 'final' else None)
        r64 = sr.compute(unit, x0, x1, form=form, region=region)
        out.append((unit, (x0, x1, region), r32, r64))
    return sr, out


def test_split_representation():
    """hi = fp16(v), lo = fp16(v - hi): the float32 sum hi + lo is exact, |v - (hi + lo)| <= rep(v) = max(2^(e-23), 2^-25), and
    both branches of the bound are attained (so no smaller formula of this shape holds)."""
    g = torch.Generator().manual_seed(5)
    mant = torch.rand(400000, generator=g, dtype=torch.float64) + 1.0
    expo = torch.randint(-30, 16, (400000,), generator=g)      # (|v| < 2^16; values that round to an infinite hi are dropped)
    sign = torch.randint(0, 2, (400000,), generator=g) * 2 - 1
    v = [(sign * torch.ldexp(mant, expo)).to(torch.float32)]
    # edges: powers of two and their float32 neighbours, ties of both roundings, fp16-subnormal lo parts (|v - hi| < 2^-14, i.e.
    # v below 2^-3), fp16-subnormal and zero hi parts, the largest finite hi
    for e in range(-30, 16):
        b = torch.tensor([2.0 ** e], dtype=torch.float32)
        near = [b, torch.nextafter(b, b * 2), torch.nextafter(b, b * 0), b * (1 + 2.0 ** -11), b * (1 + 2.0 ** -11 + 2.0 ** -23),
                b * (1 + 2.0 ** -11 - 2.0 ** -23), b * (1 + 2.0 ** -12 + 2.0 ** -23), b * (1 + 2.0 ** -12 + 2.0 ** -22),
                b * (2 - 2.0 ** -11), b * (2 - 2.0 ** -12 - 2.0 ** -23), b * (1 + 2.0 ** -10 - 2.0 ** -12 - 2.0 ** -23)]
        v += near + [-x for x in near]
    v.append(torch.tensor([0.0, 65504.0, 65519.0, 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -26, 2.0 ** -14 - 2.0 ** -38], dtype=torch.float32))
    v = torch.cat(v)
    v = v[v.abs() < 65520.0]
    hi, lo = R.split_parts(v)
    assert bool(torch.isfinite(hi).all()) and bool((lo.abs() < 2.0 ** -14).any()) and bool((hi == 0).any())
    s32 = hi + lo
    s64 = hi.to(torch.float64) + lo.to(torch.float64)
    assert torch.equal(s32.to(torch.float64), s64), 'the float32 sum of a pair is not exact'
    assert torch.equal(R.to_storage(v, 'f16x2'), s64)
    err = (v.to(torch.float64) - s64).abs()
    bound = R.rep(v.to(torch.float64).abs())
    worst = int((err / bound).argmax())
    print(f'split representation: {v.numel()} values, largest |v - (hi + lo)| / rep(v) = {float((err / bound).max()):.3f} at v = {float(v[worst])!r}')
    assert bool((err <= bound).all()), (float(v[worst]), float(err[worst]), float(bound[worst]))
    normal = bound > 2.0 ** -25
    assert bool((err[normal] == bound[normal]).any()), '2^(e-23) is never attained: the bound is not tight'
    assert bool((err[~normal] == 2.0 ** -25).any()), '2^-25 is never attained: the bound is not tight'
    # the pair of a sum is the pair it came from up to the tie case, where only the sign of lo moves: |lo| is a function of the sum
    h2, l2 = R.split_parts(s32)
    assert torch.equal(h2 + l2, s32) and torch.equal(l2.abs(), lo.abs())


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


OLD_TOL = {'f16x2': 1e-5, 'f32': 2e-5}        # test_split_/test_f32_layerwise_buffers_match_oracle: max|diff| <= tol max|tensor|


def _alive(x):
    """channels that are non-zero behind their ReLU at half of the voxels or more (a dead channel's terms are zero anyway)."""
    return [c for c in range(x.shape[0]) if float((x[c] != 0).double().mean()) >= 0.5]


def _report(sr, name, unit, what, bad, r64):
    """(elements over the rule, does the old layer-wise criterion see it) of a stand-in output with a defect; one table line."""
    nbad, _, ratio, diff = sr.check(bad, r64)
    old = float(diff.max()) > OLD_TOL[sr.act] * float(r64['ref'].abs().max())
    print(f'DEFECTTABLE | {sr.act} | {name} op {unit[1]} | {what} | elements over the rule {nbad} of {diff.numel()} | worst '
          f'{ratio:.1f} x allowed | max|diff| / max|tensor| {float(diff.max()) / float(r64["ref"].abs().max()):.1e} | '
          f'old criterion {"fails it" if old else "PASSES it"}')
    return nbad


@pytest.mark.parametrize('name,tile', [('myelin3x16', (5, 17, 19)), ('semseg_spine', (8, 16, 32)), ('mivcsj', (5, 17, 19))])
def test_split_plan_defects_fail_the_rule(name, tile):
    """Defects of a split-fp16 kernel in the stand-in (three products of the parts in float32, re-split): each changes terms of
    2^-11 of a product or less.  Planted at the first convolution with two input chunks or more that is not a GroupNorm
    producer (the composite's rule carries the statistics' slack)."""
    sr, units = _stand_in(name, tile, 'f16x2')

    def cin(k):
        d = sr.ops[units[k][0][1]]
        return d.cin0 + max(d.cin1, 0) if d.src1 >= 0 else d.cin0
    convs = [k for k, (u, _, _, _) in enumerate(units) if u[0] == 'conv' and sr.ops[u[1]].src0 != 0 and cin(k) >= 32]
    plain = [k for k in convs if units[k][0][2] < 0]
    k = (plain or convs)[0]
    unit, (x0, x1, region), r32, r64 = units[k]
    d = sr.ops[unit[1]]
    good = _stored(sr, r32)
    assert sr.check(good, r64)[0] == 0
    xin = x0 if x1 is None else torch.cat((x0[:, :x1.shape[1], :x1.shape[2], :x1.shape[3]], x1), 0)
    live = _alive(xin)
    kzc = d.kz // 2

    def run(p_hook):
        return _stored(sr, sr.compute(unit, x0, x1, dtype=torch.float32, region=region, p_hook=p_hook))

    # (1) the w_lo . x_hi pass dropped for one 16-channel chunk
    j = live[0] // 16

    def no_wlo(pairs, j=j):
        pairs[0][1][:, 16 * j:16 * j + 16] = 0.0
        return pairs
    assert _report(sr, name, unit, f'w_lo.x_hi pass dropped for chunk {j}', run(no_wlo), r64) > 0

    # (2) x_lo of one input channel read as zero at one tap
    ci = live[0]

    def no_xlo(pairs, ci=ci):
        pairs[2][1][:, ci, kzc, 1, 2] = 0.0
        return pairs
    assert _report(sr, name, unit, f'x_lo of channel {ci} zero at tap ({kzc},1,2)', run(no_xlo), r64) > 0

    # (3) the lo plane of chunk j paired with the hi plane of chunk j + 1
    def mispair(pairs):
        xl = pairs[2][0]
        xl[16:32] = xl[0:16].clone()
        return pairs
    assert _report(sr, name, unit, 'lo plane of chunk 0 paired with the hi plane of chunk 1', run(mispair), r64) > 0

    # (4) one tap missing on one face of the tile (the last column; the tap reads the column before it, inside the tile)
    def no_tap(pairs):
        for _, w in pairs:
            w[:, :, kzc, 1, 0] = 0.0
        return pairs
    bad = good.clone()
    bad[..., -1] = run(no_tap)[..., -1]
    assert _report(sr, name, unit, f'tap ({kzc},1,0) missing on the face x = W - 1', bad, r64) > 0

    # (5) the output's lo part not stored for one chunk
    bad = good.clone()
    bad[:16] = R.split_parts(r32['ref'])[0][:16].to(torch.float64)
    assert _report(sr, name, unit, 'lo part of output chunk 0 not stored', bad, r64) > 0

    # record only, no assertion: the two smallest defects at the convolution with the most terms, where one term is a smaller
    # share of S (the rule allows c 2^-24 S; a single x_lo term is at most 2^-12 of its product)
    kd = max(convs, key=lambda q: cin(q) * sr.ops[units[q][0][1]].kz * 9)
    if kd != k:
        unit, (x0, x1, region), r32, r64 = units[kd]
        kzc = sr.ops[unit[1]].kz // 2
        xin = x0 if x1 is None else torch.cat((x0[:, :x1.shape[1], :x1.shape[2], :x1.shape[3]], x1), 0)
        ci = (_alive(xin) or [0])[0]
        j = ci // 16

        def no_wlo_deep(pairs):
            pairs[0][1][:, 16 * j:16 * j + 16] = 0.0
            return pairs

        def no_xlo_deep(pairs):
            pairs[2][1][:, ci, kzc, 1, 2] = 0.0
            return pairs
        for what, hook in ((f'(record) w_lo.x_hi pass dropped for chunk {j}', no_wlo_deep),
                           (f'(record) x_lo of channel {ci} zero at tap ({kzc},1,2)', no_xlo_deep)):
            _report(sr, name, unit, what, _stored(sr, sr.compute(unit, x0, x1, dtype=torch.float32, region=region, p_hook=hook)), r64)


@pytest.mark.parametrize('name,tile', [('myelin3x16', (5, 17, 19)), ('semseg_spine', (8, 16, 32)), ('mivcsj', (5, 17, 19))])
def test_f32_plan_defects_fail_the_rule(name, tile):
    """Defects of an fp32 FMA kernel: one tap missing at one border voxel; one channel of the second source of a concatenation
    skipped.  Planted at the first convolution that reads two sources."""
    sr, units = _stand_in(name, tile, 'f32')
    k = next(k for k, (u, _, _, _) in enumerate(units) if u[0] == 'conv' and sr.ops[u[1]].src1 >= 0)
    unit, (x0, x1, region), r32, r64 = units[k]
    d = sr.ops[unit[1]]
    good = _stored(sr, r32)
    assert sr.check(good, r64)[0] == 0
    kzc = d.kz // 2

    def no_tap(w):
        w[:, :, kzc, 2, 2] = 0.0
        return w
    bad = good.clone()
    bad[:, 0, 0, 0] = _stored(sr, sr.compute(unit, x0, x1, dtype=torch.float32, region=region, w_hook=no_tap))[:, 0, 0, 0]
    assert _report(sr, name, unit, f'tap ({kzc},2,2) missing at voxel (0,0,0)', bad, r64) > 0

    ci = d.cin0 + _alive(x1)[0]

    def skip(w, ci=ci):
        w[:, ci] = 0.0
        return w
    bad = _stored(sr, sr.compute(unit, x0, x1, dtype=torch.float32, region=region, w_hook=skip))
    assert _report(sr, name, unit, f'channel {ci - d.cin0} of the second source skipped', bad, r64) > 0
