"""Time of the view network (csrc/sd_viewnet.hip) on 40 samples of the CMN geometry (20 views of 128 x 256, 4 channels), seeded weights
and synthetic views.

    python tools/celltype_probe.py [--out profiles/celltype_probe.json] [--samples 40]

Reports, as the minimum of three runs after one warm-up, from HIP events and without uploads: one ``sd_viewnet_forward`` over all samples
per storage type, the rate that the 8.3 GFLOP per sample (counted from the layer shapes, ``ViewNetSpec.flops_per_sample``) give with
it, and the time of every layer kernel and of the head kernel (``sd_viewnet_forward_timed``: an event behind every launch; the run of
three with the smallest sum).  The samples draw their planes from 160 distinct planes (5 MB): the input comes from the caches, and the
whole call is a window of a few milliseconds.  ``torch_cpu_baseline``: the float32
restatement of the tests on this host's CPU for two samples, scaled to one sample -- a baseline of the restatement, not of the reference,
which cannot run here.  No pass / fail rides on the times."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--samples', type=int, default=40)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'celltype_probe.json'))
    args = ap.parse_args()
    import torch
    import _viewnet_ref as R
    from syconn_amd import _dev as D
    from syconn_amd.cnn.viewnet_spec import CELLTYPE_CMN
    from syconn_amd.handler.prediction import ViewModel
    dev = D.device('cuda:0')
    spec, Dv, H, W, n = CELLTYPE_CMN(7, 2), 20, 128, 256, args.samples
    arrs = R.make_weights(spec, 1, Dv, H, W)
    base = R.synthetic_views(2, 8, 4, Dv, H, W)
    views = torch.from_numpy(base).to(dev)                      # 8 x 20 planes; the samples draw their planes from them
    rng = np.random.default_rng(0)
    table = torch.from_numpy(rng.integers(0, 8 * Dv, (n, Dv)).astype(np.int32)).to(dev)
    scal = torch.from_numpy(rng.uniform(0, 1, (n, 2)).astype(np.float32)).to(dev)
    res = dict(samples=n, geometry=[4, Dv, H, W], gflop_per_sample=spec.flops_per_sample(Dv, H, W) / 1e9, device=torch.cuda.get_device_name(0),
               arch=torch.cuda.get_device_properties(0).gcnArchName)
    for store in ('f16', 'bf16'):
        m = ViewModel(spec, R.state_dict_of(spec, arrs), act_dtype=store, device=dev)
        ws = D.scratch('sd_viewnet_workspace_bytes', dev, m._h, n, Dv, H, W)
        logits = torch.empty((n, 7), dtype=torch.float32, device=dev)
        flags = torch.zeros(2, dtype=torch.int32, device=dev)
        times = []
        for _ in range(4):                                      # the first run warms up
            e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            e[0].record()
            D.call('sd_viewnet_forward', dev, m._h, views, 8 * Dv, Dv, H, W, table, n, Dv, scal, logits, ws, ws.numel(), flags)
            e[1].record()
            torch.cuda.synchronize(dev)
            times.append(e[0].elapsed_time(e[1]))
        assert flags.cpu().tolist() == [0, 0] and torch.isfinite(logits).all()
        ms = min(times[1:])
        per_op = []
        for _ in range(4):
            out = (C.c_float * m.num_ops)()      # n_layers + 1 values are written
            D.L.check(D.L.load().sd_viewnet_forward_timed(*D.pointers((m._h, views, 8 * Dv, Dv, H, W, table, n, Dv, scal, logits, ws, ws.numel(), flags)),
                                                          D.stream(dev), out), 'sd_viewnet_forward_timed')
            per_op.append(list(out)[:len(spec.layers) + 1])
        best = min(per_op[1:], key=sum)
        res[store] = dict(forward_ms=ms, runs_ms=times[1:], tflops=res['gflop_per_sample'] * n / ms, workspace_mib=ws.numel() / 2 ** 20,
                          layer_ms=best[:-1], head_ms=best[-1], timed_sum_ms=sum(best))
    two = base[:2]
    t = time.perf_counter()
    R.forward32(spec, arrs, two, np.zeros((2, 2), np.float32))
    res['torch_cpu_baseline'] = dict(what='float32 restatement (tests/_viewnet_ref.py: forward32) on this host, per sample',
                                     ms_per_sample=(time.perf_counter() - t) * 500, threads=torch.get_num_threads())
    print(json.dumps(res, indent=1))
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
