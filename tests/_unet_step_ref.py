"""One op of a dense-prediction plan in float64, from the plan alone (test support; no kernel code, nothing of the
oracle's module graph).

The device path stores every activation as a bf16 / f16 number and accumulates in fp32.  `StepRef` takes the INPUT buffers of
one plan op exactly as the device stored them, computes that one op in float64 and says how far a correct device result may
be from it.  No earlier layer's rounding noise enters, so the allowed difference is half a unit in the last place of the
storage type plus the cost of fp32 accumulation -- one to two orders of magnitude below what a single wrong term produces.

What is restated, and from where
--------------------------------
* plan.py `plan_from_unet_state_dict` / `plan_from_sequential` (lines 58-180): an op is an `OpDesc` (kind, src0, src1, dst,
  cin0, cin1, cout, kz, relu, norm, groups, eps, offsets into the float32 blob).  A convolution with `src1 >= 0` reads the
  concatenation (src0, src1) in that order (plan.py:130, weight input-channel axis: `pack_conv` in sd_plan.cpp); src0 (the
  up-convolved tensor, 2x the level below) is cropped at the high end to src1's extent (`infer_shapes`, sd_plan.h).  A GROUPNORM op
  works in place on `src0`; its `src1`, if any, only lends the extent of the region (plan.py:81-83, `launch_groupnorm_op` in sd_api.hip).
* BatchNorm fold, `Builder::fold_bn` in sd_plan.cpp, in float32 and in this order: ``s = gamma / sqrt(var + eps)``,
  ``shift = beta - mean * s``; weights ``w * s`` (`wat`, `add_upconv`), bias ``b * s + shift`` (`folded_bias`; all in sd_plan.cpp).
* Weight rounding, what the packing was found to do:
  - convolutions that do not read the network input and up-convolutions: the folded float32 weight is rounded to the storage
    type (round to nearest even: `cvt` in `pack_conv` / `add_upconv`, sd_plan.cpp); the bias stays float32.  The reference rounds the same float32
    product with torch's conversion, so its weights are the device's bit for bit.
  - the FIRST convolution keeps float32 weights (`pack_first_f32`, sd_plan.cpp): `k_conv_first<... f32 MFMA chain>` multiplies them with
    ``float32(v) / 255`` (sd_kernels.hip:53) -- form ``'f32_chain'``, also the float32-input form.  A planar first
    convolution with uint8 input runs on the exact uint8 values with ``float32(float64(w) / 255)`` carried as three bf16
    parts = all 24 mantissa bits (`pack_first_u8`, sd_plan.cpp) -- form ``'u8_mfma'``; the bias is float32 in both.
  - the FINAL 1x1x1 layer: the matrix-core forms (`k_final_mfma`, `add_final`, and the final layer fused into the
    last convolution's epilogue, `fuse_final`; both pack with `pack_hilo_frags`, sd_plan.cpp) carry each float32 weight as ``hi + lo`` with ``hi = round_s(w)``,
    ``lo = round_s(w - hi)`` in the storage type: 16 mantissa bits for bf16, 22 for f16, NOT the float32 weight -- form
    ``'hilo'``.  The scalar `k_final` (float32 weights, form ``'f32'``) only runs from 481 padded input channels on
    (`launch_final`, sd_kernels.hip), which no network of the path has.  The bias is float32.
* Pooling: ceil-mode maximum over (kz, 2, 2) windows (`infer_shapes` in sd_plan.h, sd_kernels.hip:490-530): exact.
* Up-convolution: stride = kernel = (kz, 2, 2), weight layout [cin][cout][kz][2][2] (plan.py:118, `add_upconv` in sd_plan.cpp); the
  buffer holds the uncropped 2x tensor (`infer_shapes`).
* GroupNorm (sd_kernels.hip:724-913): the producer's output is rounded to storage, per-channel sums of the STORED values
  over the region become per-group mean / biased variance in double, ``scale = float32(rstd * gamma)``,
  ``shift = float32(beta - mean * rstd * gamma)``, ``y = relu(x * scale + shift)`` in fp32, rounded to storage; outside the
  region the buffer keeps the raw values (nobody reads them).  Under SD_KEEP_ALL the op runs in place, so only the composite
  producer + GroupNorm can be compared.

Everything after the rounding of the weights is float64: products, sum, bias, ReLU.

The allowed difference
----------------------
Alongside every output the module returns ``S = sum |w| |x| + |b|`` per output element (the same op on ``|x|`` with
``|w|``).  With p = 8 (bf16) / 11 (f16) and ``ulp_s(a) = 2^(floor(log2 a) - (p - 1))`` (f16: at least 2^-24):

* accumulation term ``eps = c * 2^-24 * S``;
* stored outputs: ``|dev - ref| <= ulp_s(|ref| + eps) / 2 + eps``;
* final logits (float32): ``eps`` plus half a float32 ulp of ``|ref| + eps``;
* pooling: equality;
* GroupNorm composite.  Let r be the float64 raw value, q = round_s(r) what the reference stores and q' what the device
  stores.  The device's fp32 sum is within eps of r, so q' is q or, where r lies within eps of a rounding boundary, its
  neighbour one step ulp_s(r) away.  With y = relu(scale * q + shift) this moves y by at most ``|scale| * ulp_s(|r| + eps)``
  = ``|gamma * rstd| * ulp_s(raw)`` for the element's channel and group: the flip term, allowed at every element.  The
  statistics see the same flips: only elements within eps of a boundary can flip, which bounds the change of the group's
  mean (``dm``) and second moment and through them of rstd (``dr``); the fp32 partial sums of the statistics kernels (16
  values per thread in `k_gn_stats`, at most 16 per lane in a convolution epilogue, doubles from there on) add at most
  ``64 * 2^-24`` relative to both moments.  The apply pass rounds scale and shift to float32 and does one fp32 fma:
  ``2^-23 (|scale q| + |shift|)``.  So ``E = |scale| (ulp_s(|r| + eps)) + |scale| dm + |gamma (q - mean)| dr + 2^-23 (|scale
  q| + |shift|)`` and ``|dev - ref| <= ulp_s(|ref| + E) / 2 + E``.

The constant c is measured against the reference, never against the device: ``c_ref`` is the largest
``|ref32 - ref64| / (2^-24 * S)`` over all ops of the cases of tests/test_unet_steps_cpu.py (ref32: the same op in float32
with torch-CPU), and ``c = 4 * c_ref``.  The factor covers a different summation tree (MFMA K-steps, per-chunk partial
sums); it does not cover a different precision.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

SD_OP_CONV, SD_OP_POOL, SD_OP_UPCONV, SD_OP_GROUPNORM, SD_OP_FINAL = 1, 2, 3, 4, 5      # include/syconn_dense.h

PREC = {'bf16': 8, 'f16': 11}
TORCH_DT = {'bf16': torch.bfloat16, 'f16': torch.float16}
ULP_FLOOR = {'bf16': 2.0 ** -133, 'f16': 2.0 ** -24}

# Measured by tests/test_unet_steps_cpu.py::test_accumulation_constant over its cases (myelin 3x16, semseg_spine, semseg_axon,
# mivcsj, build_cnn3; tiles (8, 16, 32) and (5, 17, 19); stand-in inputs rounded to storage): the largest
# |ref32 - ref64| / (2^-24 S) of any op, float32 side computed on one thread.  Measured 3.66 (bf16: semseg_axon's 48-term final
# layer; the 9-tap first convolution 3.17, 288-term planar layers 2.10, 6912-term 3x3x3 layers 0.51) and 5.63 (f16: a 96-term
# up-convolution of semseg_axon; 288 terms 4.08, 6912 terms 0.77): set by the ops with few terms, where every rounding of the
# float32 sum counts in full.  torch's float32 summation order depends on how it splits the work: with 2 ... 32 threads the same
# measurement gave 3.66 ... 4.46 and 4.81 ... 6.48.  Recorded: the largest seen, rounded up.
C_REF = {'bf16': 4.5, 'f16': 6.5}
C = {k: 4.0 * v for k, v in C_REF.items()}


def ulp_s(a: torch.Tensor, act: str) -> torch.Tensor:
    """Spacing of the storage type at magnitude `a` (float64, >= 0)."""
    _, e = torch.frexp(a.clamp_min(1e-300))          # a = m 2^e, m in [0.5, 1): floor(log2 a) = e - 1
    return torch.ldexp(torch.ones_like(a), e - PREC[act]).clamp_min(ULP_FLOOR[act])


def ulp_f32(a: torch.Tensor) -> torch.Tensor:
    _, e = torch.frexp(a.clamp_min(1e-300))
    return torch.ldexp(torch.ones_like(a), e - 24).clamp_min(2.0 ** -149)


def round_storage(a: torch.Tensor, act: str) -> torch.Tensor:
    """float64 -> nearest storage number (ties to even), as float64; no double rounding through float32."""
    u = ulp_s(a.abs(), act)
    return torch.round(a / u) * u


def to_storage(a: torch.Tensor, act: str) -> torch.Tensor:
    """float32 -> storage type -> float64 (the conversion the host packing and the kernels' epilogues do)."""
    return a.to(torch.float32).to(TORCH_DT[act]).to(torch.float64)


class StepRef:
    """Per-op float64 reference of a plan (`ops`, `blob` of `plan_from_model`) for storage type `act`.

    ``exact=True``: nothing is rounded and the fold is done in float64 -- the chained steps then restate the network itself
    (tests/test_unet_steps_cpu.py compares that chain with the float64 oracle)."""

    def __init__(self, ops, blob, act='bf16', exact=False):
        self.ops = list(ops)
        self.blob = np.asarray(blob, dtype=np.float32)
        self.act = act
        self.exact = exact
        self._cache = {}

    # -- the plan --------------------------------------------------------------------------------------
    def units(self):
        """[(kind, op index, index of the GroupNorm op behind it or -1)]: what can be compared with one device buffer."""
        out, i = [], 0
        while i < len(self.ops):
            d = self.ops[i]
            if d.kind in (SD_OP_CONV, SD_OP_UPCONV):
                g = -1
                if i + 1 < len(self.ops) and self.ops[i + 1].kind == SD_OP_GROUPNORM and self.ops[i + 1].src0 == d.dst:
                    g = i + 1
                out.append(('conv' if d.kind == SD_OP_CONV else 'upconv', i, g))
                i += 2 if g >= 0 else 1
                continue
            if d.kind == SD_OP_POOL:
                out.append(('pool', i, -1))
            elif d.kind == SD_OP_FINAL:
                out.append(('final', i, -1))
            elif d.kind == SD_OP_GROUPNORM:
                raise ValueError('GroupNorm op without its producer in front')
            i += 1
        return out

    def _sl(self, off, n):
        return self.blob[off:off + n]

    def _fold(self, d):
        """(scale, shift) per output channel: sd_plan.cpp `fold_bn`, float32 in the device's order (float64 if exact)."""
        ft = np.float64 if self.exact else np.float32
        if d.norm != 1:
            return np.ones(d.cout, ft), np.zeros(d.cout, ft)
        g, b, m, v = (self._sl(o, d.cout).astype(ft) for o in (d.gamma_off, d.beta_off, d.mean_off, d.var_off))
        s = (g / np.sqrt(v + ft(d.eps))).astype(ft)
        return s, (b - m * s).astype(ft)

    def weights(self, i, form=None):
        """(weight, bias) of op i as float64 tensors holding exactly the numbers the device multiplies with."""
        key = (i, form)
        if key in self._cache:
            return self._cache[key]
        d = self.ops[i]
        ft = np.float64 if self.exact else np.float32
        if d.kind == SD_OP_CONV:
            cin = d.cin0 + (d.cin1 if d.src1 >= 0 else 0)
            s, sh = self._fold(d)
            w = self._sl(d.w_off, d.cout * cin * d.kz * 9).reshape(d.cout, cin, d.kz, 3, 3).astype(ft)
            w = (w * s[:, None, None, None, None]).astype(ft)
            b = (self._sl(d.b_off, d.cout).astype(ft) * s + sh).astype(ft)
            wt = torch.from_numpy(w.astype(np.float64))
            if not self.exact:
                if d.src0 == 0:
                    if form == 'u8_mfma':
                        wt = torch.from_numpy((w.astype(np.float64) / 255.0).astype(np.float32).astype(np.float64))
                    elif form != 'f32_chain':
                        raise ValueError('first convolution: form must be "f32_chain" or "u8_mfma"')
                else:
                    wt = to_storage(torch.from_numpy(w), self.act)
        elif d.kind == SD_OP_UPCONV:
            s, sh = self._fold(d)
            w = self._sl(d.w_off, d.cin0 * d.cout * d.kz * 4).reshape(d.cin0, d.cout, d.kz, 2, 2).astype(ft)
            w = (w * s[None, :, None, None, None]).astype(ft)
            b = (self._sl(d.b_off, d.cout).astype(ft) * s + sh).astype(ft)
            wt = torch.from_numpy(w.astype(np.float64)) if self.exact else to_storage(torch.from_numpy(w), self.act)
        elif d.kind == SD_OP_FINAL:
            w = self._sl(d.w_off, d.cout * d.cin0).reshape(d.cout, d.cin0, 1, 1, 1)
            b = self._sl(d.b_off, d.cout)
            w32 = torch.from_numpy(w.copy())
            if self.exact or form == 'f32':
                wt = w32.to(torch.float64)
            elif form in (None, 'hilo'):
                hi = w32.to(TORCH_DT[self.act]).to(torch.float32)
                lo = (w32 - hi).to(TORCH_DT[self.act]).to(torch.float32)
                wt = hi.to(torch.float64) + lo.to(torch.float64)
            else:
                raise ValueError('final layer: form must be "hilo" or "f32"')
        else:
            raise ValueError('op has no weights')
        out = (wt.contiguous(), torch.from_numpy(np.asarray(b, dtype=np.float64).copy()))
        self._cache[key] = out
        return out

    # -- one unit --------------------------------------------------------------------------------------
    def first_input(self, raw: torch.Tensor, form: str) -> torch.Tensor:
        """The first convolution's operand (1, D, H, W) float64: float32(v) / 255 in float32 for uint8 input, the values
        themselves for float32 input, the integers for the 'u8_mfma' form."""
        if raw.dtype == torch.uint8:
            if form == 'u8_mfma' and not self.exact:
                return raw.to(torch.float64)[None]
            return (raw.to(torch.float32) / 255.0).to(torch.float64)[None]
        return raw.to(torch.float32).to(torch.float64)[None]

    def compute(self, unit, x0, x1=None, form=None, dtype=torch.float64, region=None, w_hook=None):
        """One unit on its input buffer(s) (C, D, H, W) -- for the first convolution `x0` is the raw tile (D, H, W).
        dtype float64: the reference; float32: the same op in float32 (`ref32`, and the CPU test's stand-in for the device).
        `region`: (d, h, w) of the GroupNorm region when the GroupNorm op has a `src1`.  `w_hook(w) -> w` edits the weights
        (planted defects).  Returns a dict: 'ref' (C, D, H, W), 'S', and for GroupNorm composites the pieces of the rule."""
        kind, i, g = unit
        d = self.ops[i]
        if kind == 'pool':
            y = F.max_pool3d(x0.to(torch.float64)[None], (d.kz, 2, 2), ceil_mode=True)[0]
            return dict(kind=kind, ref=y, S=None)
        if kind == 'conv':
            if d.src0 == 0:
                x = self.first_input(x0, form)
            else:
                x = x0.to(torch.float64)
                if x1 is not None:
                    _, dd, hh, ww = x1.shape
                    x = torch.cat((x[:, :dd, :hh, :ww], x1.to(torch.float64)), 0)
            w, b = self.weights(i, form if d.src0 == 0 else None)
            if w_hook is not None:
                w = w_hook(w.clone())
            pad = (d.kz // 2, 1, 1)
            y = F.conv3d(x.to(dtype)[None], w.to(dtype), b.to(dtype), padding=pad)[0]
            S = F.conv3d(x.abs()[None], w.abs(), b.abs(), padding=pad)[0]
        elif kind == 'upconv':
            x = x0.to(torch.float64)
            w, b = self.weights(i)
            if w_hook is not None:
                w = w_hook(w.clone())
            st = (d.kz, 2, 2)
            y = F.conv_transpose3d(x.to(dtype)[None], w.to(dtype), b.to(dtype), stride=st)[0]
            S = F.conv_transpose3d(x.abs()[None], w.abs(), b.abs(), stride=st)[0]
        elif kind == 'final':
            x = x0.to(torch.float64)
            w, b = self.weights(i, form)
            if w_hook is not None:
                w = w_hook(w.clone())
            y = F.conv3d(x.to(dtype)[None], w.to(dtype), b.to(dtype))[0]
            S = F.conv3d(x.abs()[None], w.abs(), b.abs())[0]
            return dict(kind=kind, ref=y, S=S)
        else:
            raise ValueError(kind)
        if g < 0:
            if d.relu:
                y = torch.relu(y)
            return dict(kind=kind, ref=y, S=S)
        # ---- composite: producer -> round to storage -> statistics over the stored values -> scale / shift / ReLU
        gd = self.ops[g]
        if region is not None:
            y, S = y[:, :region[0], :region[1], :region[2]], S[:, :region[0], :region[1], :region[2]]
        if d.relu:
            y = torch.relu(y)
        raw = y.to(torch.float64)
        q = raw if self.exact else (round_storage(raw, self.act) if dtype == torch.float64 else to_storage(y, self.act))
        Cn = q.shape[0]
        cpg = Cn // gd.groups
        qg = q.reshape(gd.groups, -1)
        mean = qg.mean(1)
        ex2 = (qg * qg).mean(1)
        var = (ex2 - mean * mean).clamp_min(0.0)
        rstd = 1.0 / torch.sqrt(var + float(gd.eps))
        gamma = torch.from_numpy(self._sl(gd.gamma_off, Cn).astype(np.float64))
        beta = torch.from_numpy(self._sl(gd.beta_off, Cn).astype(np.float64))
        mean_c, rstd_c = mean.repeat_interleave(cpg), rstd.repeat_interleave(cpg)
        sc, sh = rstd_c * gamma, beta - mean_c * rstd_c * gamma
        if not self.exact:
            sc, sh = sc.to(torch.float32).to(torch.float64), sh.to(torch.float32).to(torch.float64)
        v4 = (-1, 1, 1, 1)
        if dtype == torch.float64:
            out = q * sc.view(v4) + sh.view(v4)
        else:
            out = (q.to(torch.float32) * sc.to(torch.float32).view(v4) + sh.to(torch.float32).view(v4))
        if gd.relu:
            out = torch.relu(out)
        return dict(kind='gn', ref=out, S=S, raw=raw, q=q, sc=sc, sh=sh, gamma=gamma, mean=mean, rstd=rstd, ex2=ex2,
                    groups=gd.groups)

    # -- the rule --------------------------------------------------------------------------------------
    def allowed(self, res, c=None):
        """Per-element allowed |dev - ref| (float64 tensor; None for pooling: equality)."""
        act = self.act
        c = C[act] if c is None else c
        if res['kind'] == 'pool':
            return None
        ref = res['ref'].to(torch.float64).abs()
        eps = c * 2.0 ** -24 * res['S']
        if res['kind'] == 'final':
            return eps + ulp_f32(ref + eps) / 2
        if res['kind'] != 'gn':
            return ulp_s(ref + eps, act) / 2 + eps
        raw, q, sc, sh = res['raw'], res['q'], res['sc'], res['sh']
        G = res['groups']
        v4 = (-1, 1, 1, 1)
        u = ulp_s(raw.abs() + eps, act)
        # elements whose stored value can differ from the reference's: the float64 value lies within eps of a boundary
        # (boundaries are the odd multiples of u / 2: distance of raw / u to the nearest half-integer)
        t = raw / u
        can_flip = ((t - torch.floor(t) - 0.5).abs() * u <= eps).to(torch.float64)
        fg = (can_flip * u).reshape(G, -1)
        qa = q.abs().reshape(G, -1)
        dm = fg.mean(1) + 2.0 ** -18 * qa.mean(1)
        de2 = (fg * (2 * qa + fg)).mean(1) + 2.0 ** -18 * res['ex2']
        dvar = de2 + 2 * res['mean'].abs() * dm + dm * dm
        dr = 0.5 * res['rstd'] ** 3 * dvar
        cpg = q.shape[0] // G
        dm_c, dr_c, mean_c = (x.repeat_interleave(cpg).view(v4) for x in (dm, dr, res['mean']))
        E = sc.abs().view(v4) * (u + dm_c) + (res['gamma'].view(v4) * (q - mean_c)).abs() * dr_c + \
            2.0 ** -23 * ((q * sc.view(v4)).abs() + sh.abs().view(v4))
        return ulp_s(ref + E, act) / 2 + E

    def check(self, dev, res, c=None):
        """(number of elements over the rule, flat index of the worst one, its |dev - ref| / allowed, the |diff| tensor)."""
        ref = res['ref'].to(torch.float64)
        dev = dev.to(torch.float64)
        assert dev.shape == ref.shape, (tuple(dev.shape), tuple(ref.shape))
        diff = (dev - ref).abs()
        tol = self.allowed(res, c)
        if tol is None:
            bad = diff != 0
            ratio = bad.to(torch.float64) * math.inf
            ratio[~bad] = 0.0
        else:
            ratio = diff / tol
            bad = ~(diff <= tol)            # (NaN counts as over the rule)
        worst = int(torch.nan_to_num(ratio, nan=math.inf).reshape(-1).argmax())
        return int(bad.sum()), worst, float(ratio.reshape(-1)[worst]), diff


def c_ratio(ref32, ref64, S):
    """largest |ref32 - ref64| / (2^-24 S) (where S > 0)."""
    r = (ref32.to(torch.float64) - ref64).abs() / (2.0 ** -24 * S.clamp_min(1e-300))
    return float(r[S > 0].max()) if bool((S > 0).any()) else 0.0


def chain(sr: StepRef, raw: torch.Tensor, dtype=torch.float64, first_form='f32_chain', final_form=None, store=None,
          hooks=None):
    """Run the whole plan unit by unit.  `store(t) -> t` is applied to every unit's output before it is kept as a buffer
    (None: no rounding); `hooks`: {unit index: dict(w_hook=..., x_edit=..., y_edit=...)} planted defects.
    Returns (buffers {id: tensor}, logits, [(unit, inputs, result)])."""
    bufs, log, logits = {}, [], None
    for ui, unit in enumerate(sr.units()):
        kind, i, g = unit
        d = sr.ops[i]
        hk = (hooks or {}).get(ui, {})
        x0 = raw if (kind == 'conv' and d.src0 == 0) else bufs[d.src0]
        x1 = bufs[d.src1] if (kind == 'conv' and d.src1 >= 0) else None
        if 'x_edit' in hk:
            x0 = hk['x_edit'](x0)
        region = None
        if g >= 0 and sr.ops[g].src1 >= 0:
            region = tuple(bufs[sr.ops[g].src1].shape[1:])
        res = sr.compute(unit, x0, x1, form=first_form if (kind == 'conv' and d.src0 == 0) else (final_form if kind == 'final' else None),
                         dtype=dtype, region=region, w_hook=hk.get('w_hook'))
        y = res['ref']
        if 'y_edit' in hk:
            y = hk['y_edit'](y)
        log.append((unit, (x0, x1, region), res))
        if kind == 'final':
            logits = y
        else:
            bufs[d.dst] = store(y) if (store is not None and kind != 'pool') else y
    return bufs, logits, log
