"""Time of the morphology embedding (``sd_viewnet_embed``: the representation network of cnn/cnn_atn.py with the sample-tiled head) on the
view probe's cell -- 3,329 rendering locations x 2 views of 128 x 256, 4 channels -- and on one table of 20,000 locations, seeded weights
and synthetic views, with the per-sample head (``sd_viewnet_forward``) on the same inputs as the A/B.

    python tools/embedding_probe.py [--out profiles/embedding_probe.json] [--bs 800]

The views of all locations are drawn from 64 distinct synthetic locations by an index on the device (the network reads view 0 of
every location in place through the sample table, so every location is its own 128 x 256 x 4 read).  Reported per storage type, as the
minimum of three runs after one warm-up, from HIP events and without uploads, the two entries alternating in one process: the whole
call (all launch sets of `bs` locations), the time of every layer kernel and of the head kernel of one launch set
(``sd_viewnet_embed_timed`` / ``sd_viewnet_forward_timed``: an event behind every launch; of three runs the one with the smallest
sum), the head's share of that sum, and TS.  The latents of the two entries are compared bit for bit.  No pass / fail rides on the
times, and no ratio is promised: whatever comes out is what the file holds."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--bs', type=int, default=800)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'embedding_probe.json'))
    args = ap.parse_args()
    import torch
    import _embedding_ref as E
    import _viewnet_ref as R
    from syconn_amd import _dev as D
    from syconn_amd.cnn.viewnet_spec import TNET_REP
    from syconn_amd.handler.prediction import EmbeddingModel
    dev = D.device('cuda:0')
    spec, H, W, vpl, bs = TNET_REP(), 128, 256, 2, args.bs
    arrs = E.make_weights(spec, 1, H, W, exact=False)
    base = torch.from_numpy(R.synthetic_views(2, 64, 4, vpl, H, W)).to(dev)
    lib = D.L.load()
    nl = len(spec.layers)
    res = dict(geometry=[4, vpl, H, W], launch_set=bs, gflop_per_location=spec.flops_per_sample(1, H, W) / 1e9,
               head_weight_bytes=4 * sum(a * b + b for a, b in zip(spec.linear_sizes[:-1], spec.linear_sizes[1:])),
               device=torch.cuda.get_device_name(0), arch=torch.cuda.get_device_properties(0).gcnArchName, head_tile_grid=D.L.SD_VIEWNET_HEAD_TILE_GRID,
               head_grid=D.L.SD_VIEWNET_HEAD_GRID)
    rng = np.random.default_rng(0)
    for label, n in (('cell_3329', 3329), ('table_20000', 20000)):
        views = base[torch.from_numpy(rng.integers(0, 64, n)).to(dev)].contiguous()      # (n, 4, 2, H, W)
        table = (torch.arange(n, dtype=torch.int32, device=dev) * vpl).reshape(n, 1)
        out = dict(locations=n, views_mib=views.numel() / 2 ** 20)
        for store in ('f16', 'bf16'):
            m = EmbeddingModel(spec, E.state_dict_of(spec, arrs), act_dtype=store, bs=bs, device=dev)
            nb = min(bs, n)
            ws = D.scratch('sd_viewnet_workspace_bytes', dev, m._h, nb, 1, H, W)
            lat = {k: torch.empty((n, spec.n_classes), dtype=torch.float32, device=dev) for k in ('embed', 'forward')}
            flags = torch.zeros(2, dtype=torch.int32, device=dev)

            def whole(entry, dst):
                e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                e[0].record()
                for b in range(0, n, nb):
                    k = min(nb, n - b)
                    D.call(entry, dev, m._h, views, n * vpl, vpl, H, W, table[b:b + k], k, 1, None, dst[b:b + k], ws, ws.numel(), flags)
                e[1].record()
                torch.cuda.synchronize(dev)
                return e[0].elapsed_time(e[1])

            def per_launch(entry, dst):
                ms = (C.c_float * (nl + 2))()
                D.L.check(getattr(lib, entry)(*D.pointers((m._h, views, n * vpl, vpl, H, W, table[:nb], nb, 1, None, dst[:nb], ws, ws.numel(), flags)),
                                              D.stream(dev), ms), entry)
                return list(ms)[:nl + 1]

            calls = {'embed': [], 'forward': []}
            launches = {'embed': [], 'forward': []}
            for _ in range(4):                                      # the first run of each warms up; the two entries alternate
                calls['embed'].append(whole('sd_viewnet_embed', lat['embed']))
                calls['forward'].append(whole('sd_viewnet_forward', lat['forward']))
            for _ in range(4):
                launches['embed'].append(per_launch('sd_viewnet_embed_timed', lat['embed']))
                launches['forward'].append(per_launch('sd_viewnet_forward_timed', lat['forward']))
            assert flags.cpu().tolist() == [0, 0] and torch.isfinite(lat['embed']).all()
            r = dict(tile_samples=m.tile_samples, workspace_mib=ws.numel() / 2 ** 20, launch_sets=-(-n // nb),
                     bit_identical=bool(torch.equal(lat['embed'], lat['forward'])))
            for k in ('embed', 'forward'):
                best = min(launches[k][1:], key=sum)
                call_ms = min(calls[k][1:])
                r[k] = dict(call_ms=call_ms, call_runs_ms=calls[k][1:], locations_per_s=n / call_ms * 1e3, tflops=res['gflop_per_location'] * n / call_ms,
                            launch_layer_ms=best[:-1], launch_head_ms=best[-1], launch_sum_ms=sum(best), head_share=best[-1] / sum(best))
            r['head_ms_forward_over_embed'] = r['forward']['launch_head_ms'] / r['embed']['launch_head_ms']
            r['call_ms_forward_over_embed'] = r['forward']['call_ms'] / r['embed']['call_ms']
            out[store] = r
            del m, ws, lat
        res[label] = out
        del views
        torch.cuda.empty_cache()
    print(json.dumps(res, indent=1))
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
