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

The two reference-precision plans
----------------------------------
``'f16x2'`` (split-fp16 plan: sd_split.hip, k_conv_mfma MODE 3, the split forms of k_conv_first / k_upconv_*) and ``'f32'``
(fp32 FMA plan, sd_f32.hip) are the same contract with another representation.

* f16x2 values (`split_pk` in sd_device.h, `split8` in sd_split.hip): an fp32 result v is stored as ``hi = fp16(v)``,
  ``lo = fp16(v - hi)``, both round to nearest even; `sd_debug_read_buffer` returns ``float32(hi) + float32(lo)``
  (`k_read_buffer_split`).  With e = floor(log2 |v|): ``|v - hi| <= 2^(e-11)`` and ``v - hi`` is exact in fp32, a multiple of
  2^(e-23) -- at most 13 significant bits, of which fp16 keeps 11 only when ``|v - hi| >= 2^(e-12)``, so the second rounding
  loses at most one bit worth 2^(e-23); a `lo` below 2^-14 is an fp16 subnormal, a multiple of 2^-24, and loses at most
  2^-25.  Hence ``|v - (hi + lo)| <= rep(v) = max(2^(e-23), 2^-25)``, half of the 2^(e-22) a looser count gives;
  tests/test_unet_steps_cpu.py::test_split_representation pins the bound, that it is attained, and that the float32 sum
  ``hi + lo`` is exact.  In the rule ``ulp_s = 2 rep``, so that ``ulp_s / 2`` is the representation error.
* f16x2 weights (`pack_conv`, `add_upconv`, `split_scale`, `split_part` in sd_plan.cpp): the folded float32 weight w is scaled
  by the layer's power of two 2^k, k = 14 - floor(log2 max|w|) (clamped to +-60), then ``hi = fp16(w 2^k)``,
  ``lo = fp16(w 2^k - hi)``; the bias is float32 times 2^k and the epilogue multiplies by 2^-k (all exact).  The reference
  multiplies with ``(hi + lo) 2^-k``.  The device sums three products ``w_lo x_hi + w_hi x_hi + w_hi x_lo`` (virtual
  chunks [hi | hi | lo] against weight groups [lo | hi | hi]) into one fp32 accumulator; the fourth, ``w_lo x_lo``, is
  dropped: ``D = sum |w_lo| |x_lo| 2^-k`` per output element, computed from the parts.  The first convolution keeps folded
  float32 weights (`pack_first_f32`; `k_conv_first<split-fp16, f32 MFMA chain>`) -- form ``'f32_chain'``, D = 0.  The final
  layer: `k_final_split` (its own launch) runs an fp32 FMA chain on the float32 weights -- form ``'f32'``, D = 0; in the planar
  convolution's epilogue (`fuse_final`, `pack_hilo_frags` with `fscale`) the weights are fp16 hi / lo parts of ``w 2^k`` with k
  from the largest |w|, three products again, then one ``fmaf(acc, 2^-k, bias)`` -- form ``'hilo'``.
* f16x2 pooling (`k_maxpool_split`, the convolution epilogue, `k_gn_apply_pool_split`): the maximum of the exact sums, re-split
  -- the pair it came from: equality of the read-back sums.
* f16x2 GroupNorm (`k_gn_stats_split` / the MODE 3 epilogue, `k_gn_finalize`, `k_gn_apply_split`): statistics of the exact
  sums hi + lo (fp32 partials of at most 64 values, double from there on), scale / shift as in the other plans, one fp32
  ``fmaf``, re-split.
* f32 (sd_f32.hip): activations are float32 with the real channel count.  `f32_model_create` does NOT fold the BatchNorm into
  the weights: `k32_conv` and `k32_upconv` compute ``(sum w x + b) * alpha + beta'`` with the float32 network weights,
  ``alpha = gamma / sqrt(var + eps)`` and ``beta' = beta - mean * alpha`` in float32 (the operations of `fold_bn`, applied to the
  sum and not to the weights), then ReLU.  The reference does the same in float64 on those float32 numbers and
  ``S = (sum |w| |x| + |b|) |alpha| + |beta'|``.  `k32_final`: fp32 FMA chain on the float32 weights, bias added last.
  `k32_pool`: exact.  `k32_gn_stats` sums the float32 values in double; `k32_gn_apply` takes ``scale = float32(rstd) *
  gamma``, ``shift = beta - scale * float32(mean)`` and ``v = x * scale + shift`` in fp32: rounding of rstd and of the
  product 2^-23 |scale|, of the mean, the product and the difference 2^-24 (2 |scale mean| + |shift|), of the apply
  2^-24 (|x scale| + |v|) -- together at most ``2^-22 |x scale| + 2^-21 |scale mean| + 2^-23 |beta|``.
* allowed difference: ``eps = c 2^-24 S + D`` (D = 0 for f32); stored outputs ``|dev - ref| <= ulp_s(|ref| + eps) / 2 + eps``
  with ulp_s / 2 = rep (f16x2) or half a float32 ulp (f32); logits as above; pooling equality.
* GroupNorm composite: these representations are finer than the accumulation term, so the picture of the 16-bit types -- the
  stored value is the reference's or its neighbour -- does not hold: EVERY raw value the device stores may be
  ``delta = eps + ulp_s(|r| + eps)`` away from the float64 raw value r (which the reference normalises unrounded).  The
  rule is the E above with that delta in place of the flip term, at every element, in the statistics too:
  ``E = |scale| (delta + dm) + |gamma (r - mean)| dr + apply`` with dm, dr from delta as above (f32: no fp32 partial sums)
  and ``apply = 2^-23 (|scale r| + |shift|)`` (f16x2) or the f32 term above; ``|dev - ref| <= ulp_s(|ref| + E) / 2 + E``.

The constant c is measured against the reference, never against the device: ``c_ref`` is the largest
``|ref32 - ref64| / (2^-24 * S)`` over all ops of the cases of tests/test_unet_steps_cpu.py (ref32: the same op in float32
with torch-CPU), and ``c = 4 * c_ref``.  The factor covers a different summation tree (MFMA K-steps, per-chunk partial
sums); it does not cover a different precision.  For f16x2 ref32 is the sum of the three products in float32 (so the dropped
fourth product is inside c_ref as well as in D: at most 2^-24 S, i.e. 1 of c_ref); for f32 the float32 sequence of `k32_conv`.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

SD_OP_CONV, SD_OP_POOL, SD_OP_UPCONV, SD_OP_GROUPNORM, SD_OP_FINAL = 1, 2, 3, 4, 5      # include/syconn_dense.h

PREC = {'bf16': 8, 'f16': 11}
TORCH_DT = {'bf16': torch.bfloat16, 'f16': torch.float16}
ULP_FLOOR = {'bf16': 2.0 ** -133, 'f16': 2.0 ** -24}
REFPREC = ('f16x2', 'f32')          # the reference-precision plans: no 16-bit storage type
# relative error of the fp32 partial sums in front of the double GroupNorm statistics (f32: k32_gn_stats sums doubles)
STAT_REL = {'bf16': 2.0 ** -18, 'f16': 2.0 ** -18, 'f16x2': 2.0 ** -18, 'f32': 2.0 ** -50}

# Measured by tests/test_unet_steps_cpu.py::test_accumulation_constant over its cases (myelin 3x16, semseg_spine, semseg_axon,
# mivcsj, build_cnn3; tiles (8, 16, 32) and (5, 17, 19); stand-in inputs rounded to storage): the largest
# |ref32 - ref64| / (2^-24 S) of any op, float32 side computed on one thread.  Measured 3.66 (bf16: semseg_axon's 48-term final
# layer; the 9-tap first convolution 3.17, 288-term planar layers 2.10, 6912-term 3x3x3 layers 0.51) and 5.63 (f16: a 96-term
# up-convolution of semseg_axon; 288 terms 4.08, 6912 terms 0.77): set by the ops with few terms, where every rounding of the
# float32 sum counts in full.  torch's float32 summation order depends on how it splits the work: with 2 ... 32 threads the same
# measurement gave 3.66 ... 4.46 and 4.81 ... 6.48.  Recorded: the largest seen, rounded up.
# f16x2 / f32, same cases and stand-in inputs rounded to the representation, one thread: 8.97 (f16x2: a 64-term up-convolution of
# semseg_spine, whose three products are 192 float32 terms; 96 terms 8.91, the 48-term final layer in its hi / lo form 6.99,
# 432-term planar layers 4.67, 6912-term 3x3x3 layers 1.89, the float32 first convolution 3.17) and 5.06 (f32: a 96-term
# up-convolution of mivcsj; 288-term planar layers 4.93, 6912 terms 0.66; the affine behind the sum is inside).  With 2, 4 and 8
# threads: 8.69, 8.85, 9.30 and 5.08, 5.01, 5.10.  Recorded: the largest seen, rounded up.
C_REF = {'bf16': 4.5, 'f16': 6.5, 'f16x2': 9.5, 'f32': 5.5}
C = {k: 4.0 * v for k, v in C_REF.items()}


def rep(a: torch.Tensor) -> torch.Tensor:
    """Largest |v - (hi + lo)| of the split-fp16 pair of an fp32 value of magnitude `a` (float64, >= 0): max(2^(e-23), 2^-25)."""
    _, e = torch.frexp(a.clamp_min(1e-300))
    return torch.ldexp(torch.ones_like(a), e - 24).clamp_min(2.0 ** -25)


def split_parts(v: torch.Tensor):
    """float32 -> (hi, lo) as float32 holding fp16 numbers: hi = fp16(v), lo = fp16(v - hi) (`split_pk`, `split_part`)."""
    v = v.to(torch.float32)
    hi = v.to(torch.float16).to(torch.float32)
    return hi, (v - hi).to(torch.float16).to(torch.float32)


def split_scale_exp(maxabs: float) -> int:
    """k of the layer's weight scale 2^k (`split_scale`, sd_plan.cpp): the largest |w| into [2^14, 2^15)."""
    if not (maxabs > 0.0) or not math.isfinite(maxabs):
        return 0
    return max(-60, min(60, 14 - (math.frexp(maxabs)[1] - 1)))


def ulp_s(a: torch.Tensor, act: str) -> torch.Tensor:
    """Spacing of the storage type at magnitude `a` (float64, >= 0); f16x2: twice the representation error."""
    if act == 'f16x2':
        return 2.0 * rep(a)
    if act == 'f32':
        return ulp_f32(a)
    _, e = torch.frexp(a.clamp_min(1e-300))          # a = m 2^e, m in [0.5, 1): floor(log2 a) = e - 1
    return torch.ldexp(torch.ones_like(a), e - PREC[act]).clamp_min(ULP_FLOOR[act])


def ulp_f32(a: torch.Tensor) -> torch.Tensor:
    _, e = torch.frexp(a.clamp_min(1e-300))
    return torch.ldexp(torch.ones_like(a), e - 24).clamp_min(2.0 ** -149)


def round_storage(a: torch.Tensor, act: str) -> torch.Tensor:
    """float64 -> nearest storage number (ties to even), as float64; no double rounding through float32 (the reference-
    precision types ARE functions of the fp32 value)."""
    if act in REFPREC:
        return to_storage(a.to(torch.float32), act)
    u = ulp_s(a.abs(), act)
    return torch.round(a / u) * u


def to_storage(a: torch.Tensor, act: str) -> torch.Tensor:
    """float32 -> storage type -> float64 (the conversion the host packing and the kernels' epilogues do)."""
    if act == 'f32':
        return a.to(torch.float32).to(torch.float64)
    if act == 'f16x2':
        hi, lo = split_parts(a)
        return (hi + lo).to(torch.float64)         # (the float32 sum `sd_debug_read_buffer` returns)
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
        self._parts = {}          # f16x2: (op, form) -> (w_hi, w_lo, k): the fp16 parts of w 2^k as float64
        self.split = act == 'f16x2' and not exact
        self.plain32 = act == 'f32' and not exact

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
            if self.plain32:      # the network's weights and bias; the BatchNorm affine stays behind the sum (`affine`)
                wt = torch.from_numpy(self._sl(d.w_off, d.cout * cin * d.kz * 9).reshape(d.cout, cin, d.kz, 3, 3).astype(np.float64))
                b = self._sl(d.b_off, d.cout)
            elif self.split:
                if d.src0 == 0:
                    if form != 'f32_chain':
                        raise ValueError('split plan, first convolution: form must be "f32_chain"')
                else:
                    wt = self._split_weight(key, w)
            elif not self.exact:
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
            if self.plain32:
                wt = torch.from_numpy(self._sl(d.w_off, d.cin0 * d.cout * d.kz * 4).reshape(d.cin0, d.cout, d.kz, 2, 2).astype(np.float64))
                b = self._sl(d.b_off, d.cout)
            elif self.split:
                wt = self._split_weight(key, w)
            else:
                wt = torch.from_numpy(w.astype(np.float64)) if self.exact else to_storage(torch.from_numpy(w), self.act)
        elif d.kind == SD_OP_FINAL:
            w = self._sl(d.w_off, d.cout * d.cin0).reshape(d.cout, d.cin0, 1, 1, 1)
            b = self._sl(d.b_off, d.cout)
            w32 = torch.from_numpy(w.copy())
            if self.exact or form == 'f32' or (self.plain32 and form is None):
                wt = w32.to(torch.float64)
            elif self.plain32:
                raise ValueError('fp32 plan, final layer: form must be "f32"')
            elif self.split:
                if form != 'hilo':
                    raise ValueError('split plan, final layer: form must be "f32" (k_final_split) or "hilo" (fused)')
                wt = self._split_weight(key, w32.numpy())
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

    def _split_weight(self, key, w):
        """float32 weights -> (hi + lo) 2^-k as float64; the parts are kept for D and for the three-product stand-in."""
        w = np.asarray(w, dtype=np.float32)
        k = split_scale_exp(float(np.abs(w).max()) if w.size else 0.0)
        hi, lo = split_parts(torch.from_numpy(np.ldexp(w, k).astype(np.float32)))       # (w 2^k: exact)
        hi, lo = hi.to(torch.float64), lo.to(torch.float64)
        self._parts[key] = (hi, lo, k)
        return (hi + lo) * 2.0 ** -k

    def affine(self, i):
        """f32 plan: (alpha, beta') of op i behind its sum (`affine` in f32_model_create), float32 numbers as float64."""
        a, b = self._fold(self.ops[i])
        return torch.from_numpy(a.astype(np.float64)), torch.from_numpy(b.astype(np.float64))

    def _sum(self, op, key, x, w, b, dtype, w_hook, p_hook, bias_inside=True):
        """(y, S, D) of one product sum; `op(x, w, b)` is the torch call on (1, C, ...) inputs, channel axis `op.cin_axis` of w.
        float64: the reference.  float32: the same op in float32 -- for the split plan the three products of the parts in one
        accumulation, scaled bias inside, times 2^-k (`p_hook(pairs) -> pairs` edits the (x part, w part) pairs: defects)."""
        S = op(x.abs(), w.abs(), b.abs())
        D = None
        parts = self._parts.get(key) if self.split else None
        if parts is not None:
            wh, wl, k = parts
            xh, xl = split_parts(x)
            if not torch.equal(xl.to(torch.float16).to(torch.float32), xl):
                raise ValueError('input is not the sum of an fp16 pair')
            D = op(xl.to(torch.float64).abs(), wl.abs(), None) * 2.0 ** -k
            if dtype == torch.float32:
                if w_hook is not None:
                    wh, wl = w_hook(wh.clone()), w_hook(wl.clone())
                pairs = [(xh, wl), (xh, wh), (xl, wh)]
                if p_hook is not None:
                    pairs = p_hook([(a.clone(), c.clone()) for a, c in pairs])
                xc = torch.cat([a.to(torch.float32) for a, _ in pairs], 0)
                wc = torch.cat([c.to(torch.float32) for _, c in pairs], op.cin_axis)
                b32 = b.to(torch.float32)
                if bias_inside:
                    return op(xc, wc, b32 * 2.0 ** k) * 2.0 ** -k, S, D
                return op(xc, wc, None) * 2.0 ** -k + b32.view(-1, 1, 1, 1), S, D
        if w_hook is not None:
            w = w_hook(w.clone())
        return op(x.to(dtype), w.to(dtype), b.to(dtype)), S, D

    # -- one unit --------------------------------------------------------------------------------------
    def first_input(self, raw: torch.Tensor, form: str) -> torch.Tensor:
        """The first convolution's operand (1, D, H, W) float64: float32(v) / 255 in float32 for uint8 input, the values
        themselves for float32 input, the integers for the 'u8_mfma' form."""
        if raw.dtype == torch.uint8:
            if form == 'u8_mfma' and not self.exact:
                return raw.to(torch.float64)[None]
            return (raw.to(torch.float32) / 255.0).to(torch.float64)[None]
        return raw.to(torch.float32).to(torch.float64)[None]

    def compute(self, unit, x0, x1=None, form=None, dtype=torch.float64, region=None, w_hook=None, p_hook=None):
        """One unit on its input buffer(s) (C, D, H, W) -- for the first convolution `x0` is the raw tile (D, H, W).
        dtype float64: the reference; float32: the same op in float32 (`ref32`, and the CPU test's stand-in for the device).
        `region`: (d, h, w) of the GroupNorm region when the GroupNorm op has a `src1`.  `w_hook(w) -> w` edits the weights,
        `p_hook` the pairs of the split plan's three products (planted defects).  Returns a dict: 'ref' (C, D, H, W), 'S',
        'D' (split plan: the dropped product, else None) and for GroupNorm composites the pieces of the rule."""
        kind, i, g = unit
        d = self.ops[i]
        if kind == 'pool':
            y = F.max_pool3d(x0.to(torch.float64)[None], (d.kz, 2, 2), ceil_mode=True)[0]
            return dict(kind=kind, ref=y, S=None, D=None)
        if kind == 'conv':
            wform = form if d.src0 == 0 else None
            if d.src0 == 0:
                x = self.first_input(x0, form)
            else:
                x = x0.to(torch.float64)
                if x1 is not None:
                    _, dd, hh, ww = x1.shape
                    x = torch.cat((x[:, :dd, :hh, :ww], x1.to(torch.float64)), 0)
            pad = (d.kz // 2, 1, 1)

            def op(xx, ww, bb):
                return F.conv3d(xx[None], ww, bb, padding=pad)[0]
            op.cin_axis = 1
        elif kind == 'upconv':
            wform = None
            x = x0.to(torch.float64)
            st = (d.kz, 2, 2)

            def op(xx, ww, bb):
                return F.conv_transpose3d(xx[None], ww, bb, stride=st)[0]
            op.cin_axis = 0
        elif kind == 'final':
            wform = form
            x = x0.to(torch.float64)

            def op(xx, ww, bb):
                return F.conv3d(xx[None], ww, bb)[0]
            op.cin_axis = 1
        else:
            raise ValueError(kind)
        w, b = self.weights(i, wform)
        y, S, D = self._sum(op, (i, wform), x, w, b, dtype, w_hook, p_hook, bias_inside=kind != 'final')
        if kind == 'final':
            return dict(kind=kind, ref=y, S=S, D=D)
        if self.plain32:          # (sum + b) * alpha + beta', the sequence of k32_conv / k32_upconv
            al, be = self.affine(i)
            v4 = (-1, 1, 1, 1)
            y = y * al.to(dtype).view(v4) + be.to(dtype).view(v4)
            S = S * al.abs().view(v4) + be.abs().view(v4)
        if g < 0:
            if d.relu:
                y = torch.relu(y)
            return dict(kind=kind, ref=y, S=S, D=D)
        # ---- composite: producer -> round to storage -> statistics over the stored values -> scale / shift / ReLU
        gd = self.ops[g]
        if region is not None:
            y, S = y[:, :region[0], :region[1], :region[2]], S[:, :region[0], :region[1], :region[2]]
            D = None if D is None else D[:, :region[0], :region[1], :region[2]]
        if d.relu:
            y = torch.relu(y)
        raw = y.to(torch.float64)
        # (reference-precision types: the float64 reference normalises the unrounded raw values, see the module docstring)
        q = raw if (self.exact or (self.act in REFPREC and dtype == torch.float64)) else \
            (round_storage(raw, self.act) if dtype == torch.float64 else to_storage(y, self.act))
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
        return dict(kind='gn', ref=out, S=S, D=D, raw=raw, q=q, sc=sc, sh=sh, gamma=gamma, beta=beta, mean=mean, rstd=rstd,
                    ex2=ex2, groups=gd.groups)

    # -- the rule --------------------------------------------------------------------------------------
    def allowed(self, res, c=None):
        """Per-element allowed |dev - ref| (float64 tensor; None for pooling: equality)."""
        act = self.act
        c = C[act] if c is None else c
        if res['kind'] == 'pool':
            return None
        ref = res['ref'].to(torch.float64).abs()
        eps = c * 2.0 ** -24 * res['S']
        if res.get('D') is not None:
            eps = eps + res['D']
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
        # (reference-precision types: every stored raw value may be eps + u away from the float64 one)
        step = (eps + u) if act in REFPREC else u
        fg = (step if act in REFPREC else can_flip * u).reshape(G, -1)
        qa = q.abs().reshape(G, -1)
        dm = fg.mean(1) + STAT_REL[act] * qa.mean(1)
        de2 = (fg * (2 * qa + fg)).mean(1) + STAT_REL[act] * res['ex2']
        dvar = de2 + 2 * res['mean'].abs() * dm + dm * dm
        dr = 0.5 * res['rstd'] ** 3 * dvar
        cpg = q.shape[0] // G
        dm_c, dr_c, mean_c = (x.repeat_interleave(cpg).view(v4) for x in (dm, dr, res['mean']))
        if act == 'f32':          # k32_gn_apply: float32(rstd) * gamma, beta - scale * float32(mean), x * scale + shift
            apply = 2.0 ** -22 * (q * sc.view(v4)).abs() + (2.0 ** -21 * (sc.view(v4) * mean_c).abs() +
                                                                2.0 ** -23 * res['beta'].abs().view(v4))
        else:
            apply = 2.0 ** -23 * ((q * sc.view(v4)).abs() + sh.abs().view(v4))
        E = sc.abs().view(v4) * (step + dm_c) + (res['gamma'].view(v4) * (q - mean_c)).abs() * dr_c + apply
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
