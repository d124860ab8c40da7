"""Time the temporal convs of conv2 / conv3 / conv4 the way the batch-BN
forward runs them (statistics on, BN on load, videos of 15 and 1 clips
alternating, so that blocks hold several videos): every h3 candidate with
per-clip tiles ("pc") and every h3t variant in its stacked, tap-skipping form
("stk", rnb_conv_h3t_form), in interleaved rounds, best round kept.

    python scripts/h3t_form_bench.py --cases k8,k14 --clips 128,64,32,16,1

Prints one line per (case, clips, config, form): ms and, for the h3t
variants, the grid and its rounds of 256 CUs x blocks per CU
(profiles/r8_h3t_stacked_layers.txt)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

CASES = {
    "k4": (144, 64, (8, 56, 56)),
    "k8": (288, 128, (4, 28, 28)),
    "k14": (576, 256, (2, 14, 14)),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", default="128,16,1")
    ap.add_argument("--cases", default="k8,k14")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=4)
    args = ap.parse_args()
    from rnb_amd.ops.conv import ConvGeom
    from rnb_amd.ops.conv_f32 import (F32_ALIGN, H3T_BASE, WINO_ALL, ConvLayerF32, is_h3, is_h3t,
                                      is_x6d)
    from rnb_amd.ops.native import kernels
    kk = kernels()
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev)
    k, s, p = (3, 1, 1), (1, 1, 1), (1, 0, 0)
    for name in args.cases.split(","):
        cin, cout, (T, H, W) = CASES[name]
        g = torch.Generator().manual_seed(0)
        w = torch.randn((cout, cin) + k, generator=g) * (2.0 / (cin * 3)) ** 0.5
        geom = ConvGeom(cin=cin, cout=cout, kernel=k, stride=s, padding=p, align=F32_ALIGN,
                        cin_pad=((cin + 15) // 16 * 16 if cin % 16 else 0))
        layer = ConvLayerF32(w, torch.zeros(cout), geom, False, dev, name)
        for n in [int(c) for c in args.clips.split(",")]:
            x = torch.randn((n, T, H, W, geom.cin_p), generator=g).to(dev)
            x[..., cin:] = 0
            y = torch.empty(layer.out_shape(x.shape), device=dev)
            # videos of 15 and 1 clips
            segl, v = [], 0
            while len(segl) < n:
                segl += [v] * (15 if v % 2 == 0 else 1)
                v += 1
            segl = segl[:n]
            nvid = segl[-1] + 1
            seg = torch.tensor(segl, dtype=torch.int32, device=dev)
            sums = torch.zeros((nvid, 2, geom.cout_p), dtype=torch.float64, device=dev)
            ss = torch.ones((nvid, 2, geom.cin_p), dtype=torch.float32, device=dev)
            ss[:, 1] = 0.1
            kk.conv_h3t_form(-1)
            cands = [c for c in layer.candidates(x.shape) if is_h3(c)
                     and layer.affine_ok(c, x.shape)]
            entries = []
            for c in cands:
                if is_h3t(c):
                    v_ = c - H3T_BASE
                    if kk.conv_h3t_pixels(v_, T) > 0:
                        entries.append(("pc", c, -1))
                    kk.conv_h3t_form(1)
                    if kk.conv_h3t_stacked(v_, n, T, H, W, geom.cout_p):
                        entries.append(("stk", c, 1))
                    kk.conv_h3t_form(-1)
                else:
                    entries.append(("pc", c, -1))

            def run(e):
                kk.conv_h3t_form(e[2])
                o = (sums, seg) if (e[1] in WINO_ALL or is_x6d(e[1])) else None
                layer._launch_all(x, y, None, e[1], stream, in_affine=(ss, seg), out_stats=o)

            ok = []
            for e in entries:
                try:
                    run(e)
                    ok.append(e)
                except Exception as ex:
                    print("  %s %s: %s" % (name, e, ex), flush=True)
            torch.cuda.synchronize()
            times = {}
            for rnd in range(args.rounds):
                for e in (ok if rnd % 2 == 0 else ok[::-1]):
                    run(e)
                    st, en = (torch.cuda.Event(enable_timing=True),
                              torch.cuda.Event(enable_timing=True))
                    st.record()
                    for _ in range(args.reps):
                        run(e)
                    en.record()
                    en.synchronize()
                    t = st.elapsed_time(en) / args.reps
                    times[e] = min(times.get(e, t), t)
            for e in sorted(times, key=times.get):
                extra = ""
                if is_h3t(e[1]):
                    kk.conv_h3t_form(e[2])
                    v_ = e[1] - H3T_BASE
                    blocks = kk.conv_h3t_blocks(v_, n, T, H, W, geom.cout_p)
                    rb = 256 * kk.conv_h3t_occupancy(v_, e[2] > 0)
                    extra = "blocks %5d rounds %.2f" % (blocks, blocks / rb)
                print("%-4s N=%-3d T=%d cid %4d %-3s %8.4f ms  %s"
                      % (name, n, T, e[1], e[0], times[e], extra), flush=True)
            kk.conv_h3t_form(0)
            print(flush=True)


if __name__ == "__main__":
    main()
