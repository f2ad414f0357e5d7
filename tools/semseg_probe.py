"""Times of the FCN semantic-segmentation network (csrc/sd_fcn.hip), FCN_VGG13(5) with 4 input channels, seeded weights and synthetic
views, for both storage types at the two geometries of the compartment step:

    spiness   2 views of 128 x 256 (one rendering location), and 10 (five locations: one launch set of ``predict_labels``)
    axon      1 view of 512 x 1024 (``ws = [1024, 512]``)

    python tools/semseg_probe.py [--out profiles/semseg_probe.json]

Reports, from HIP events and without uploads, the minimum of three runs after one warm-up of one ``sd_fcn_forward`` (labels only), the
rate the multiply-adds counted from the shapes (``FcnSpec.macs_per_view``) give with it, and the time of every op
(``sd_fcn_forward_timed``: an event behind the launches of every op -- a decoder step is four launches, one per output parity --; the run
of three with the smallest sum).  ``deep_share``: the share of the per-op times that block 5 and the first two decoder steps take --
the layers whose planes (4 x 8 and 8 x 16 at 128 x 256) fill a fraction of an 8 x 32 tile, which is what running an M tile over several
planes would address.  Not measured: the rendering around the network, and any reference implementation, which cannot run here.  No pass / fail rides on the times."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'semseg_probe.json'))
    args = ap.parse_args()
    import torch
    import _fcn_ref as R
    from syconn_amd import _dev as D
    from syconn_amd.cnn.fcn_spec import FCN_VGG13
    from syconn_amd.handler.prediction import SemsegViewModel
    dev = D.device('cuda:0')
    spec = FCN_VGG13(5)
    arrs = R.make_weights(spec, 1, 128, 256)
    names = [f'conv{b + 1}_{j + 1}' for b, blk in enumerate(spec.blocks) for j in range(len(blk))] + [f'deconv{i}' for i in range(1, 6)] + ['classifier']
    deep = [i for i, n in enumerate(names) if n.startswith('conv5') or n in ('deconv1', 'deconv2')]
    res = dict(net='FCN_VGG13(5), 4 input channels', ops=names, device=torch.cuda.get_device_name(0), arch=torch.cuda.get_device_properties(0).gcnArchName)
    for geom, (n_loc, nb_views, H, W) in (('spiness_128x256x2', (1, 2, 128, 256)), ('spiness_128x256x10', (5, 2, 128, 256)), ('axon_512x1024x1', (1, 1, 512, 1024))):
        views = torch.from_numpy(R.synthetic_views(2, n_loc, 4, nb_views, H, W)).to(dev)
        n = n_loc * nb_views
        gmac = spec.macs_per_view(H, W) * n / 1e9
        res[geom] = dict(planes=n, gmac=gmac)
        for store in ('f16', 'bf16'):
            m = SemsegViewModel(spec, R.state_dict_of(spec, arrs), act_dtype=store, device=dev)
            ws = D.scratch('sd_fcn_workspace_bytes', dev, m._h, n, H, W)
            labels = torch.empty((n, H, W), dtype=torch.uint8, device=dev)
            flags = torch.zeros(1, dtype=torch.int32, device=dev)
            call = (m._h, views, n, nb_views, H, W, 0, n, labels, None, ws, ws.numel(), flags)
            times = []
            for _ in range(4):                                      # the first run warms up
                e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                e[0].record()
                D.call('sd_fcn_forward', dev, *call)
                e[1].record()
                torch.cuda.synchronize(dev)
                times.append(e[0].elapsed_time(e[1]))
            assert flags.cpu().tolist() == [0]
            per_op = []
            for _ in range(4):
                out = (C.c_float * m.num_ops)()
                D.L.check(D.L.load().sd_fcn_forward_timed(*D.pointers(call), D.stream(dev), out), 'sd_fcn_forward_timed')
                per_op.append(list(out))
            best = min(per_op[1:], key=sum)
            ms = min(times[1:])
            res[geom][store] = dict(forward_ms=ms, runs_ms=times[1:], tmac_per_s=gmac / ms, workspace_mib=ws.numel() / 2 ** 20, op_ms=best,
                                    timed_sum_ms=sum(best), deep_share=sum(best[i] for i in deep) / sum(best))
    print(json.dumps(res, indent=1))
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
