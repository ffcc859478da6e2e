"""Timing of the tri-plane model's input gradient (csrc/points_grad.hip) on one GPU, one process, three alternations, minima
reported; writes profiles/points_grad.txt (appended below the accuracy figures kept there by hand).

    python tools/points_grad_time.py [--out FILE] [--points P]

At 2^19 points on bench.py's synthetic scene (800^2 position planes, a 32^2 view plane, channel-last), planes and decoder training:
  kernel      nvsr_triplane_points_grad alone on seeded rows (three position planes + the view plane): ms, and GB/s over the bytes it must move
              (3 x (4 texels + a row) x 192 B per point + a view row and 4 view texels per ray + the outputs)
  backward    the backward of (model(x) * g).sum() per arithmetic, with x.requires_grad (the rows route + the new kernel) and without (today's
              route, atomic scatter); forward excluded"""
import os
import sys

ARGV = sys.argv[1:]
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)


def main():
    import torch

    import nvsr_amd
    from bench import make_synthetic_scene

    out_path = ARGV[ARGV.index("--out") + 1] if "--out" in ARGV else os.path.join(HERE, "profiles", "points_grad.txt")
    P = int(ARGV[ARGV.index("--points") + 1]) if "--points" in ARGV else 1 << 19
    assert torch.cuda.is_available(), "points_grad_time.py measures on a GPU; there is nothing to report without one"
    dev = "cuda:0"
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def timed(fn, reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / reps

    def alternate(fns, reps):
        for f in fns.values():
            f()
        torch.cuda.synchronize()
        ms = {k: [] for k in fns}
        for _ in range(3):
            for k, f in fns.items():
                ms[k].append(timed(f, reps))
        return {k: min(v) for k, v in ms.items()}

    mc, _, sid, _ = make_synthetic_scene(dev, seed=3, channels_last=True)
    for n, p in mc.named_parameters():
        p.requires_grad_("rot_mats" not in n)
    mc.train()
    g = torch.Generator(device=dev).manual_seed(7)
    d = torch.randn(P, 3, device=dev, generator=g)
    x = torch.cat([torch.rand(P, 3, device=dev, generator=g) * 7 - 3.5, d / d.norm(dim=-1, keepdim=True)], -1)
    cot = torch.randn(P, 4, device=dev, generator=g)
    say("input gradient of the tri-plane model, %d points, 800^2 position planes, 32^2 view plane (%s)" % (P, torch.cuda.get_device_name(0)))

    planes, consts = mc.scene_args()
    rays = torch.zeros(P, 11, device=dev)
    rays[:, 0:3], rays[:, 8:11] = x[:, 0:3], x[:, 3:6]
    z = torch.zeros(P, 1, device=dev)
    rows = [torch.randn(P, 48, device=dev, generator=g) for _ in range(3)]
    view_rows = torch.randn(P, 48, device=dev, generator=g)
    op = torch.ops.nvsr.triplane_points_grad
    ms = alternate({"kernel": lambda: op(planes, consts, rays, z, rows, view_rows)}, 20)["kernel"]
    moved = P * (3 * 5 * 192 + 5 * 192 + 11 * 4 + 4 + 24)
    say("  kernel (positions + view directions, operator call)   %7.3f ms   %6.0f GB/s over %.2f GB" % (ms, moved / ms / 1e6, moved / 1e9))

    for arithmetic in ("f16x2", "bf16x3"):
        mc.arithmetic = arithmetic

        def backward(x_grad):
            xi = x.detach().requires_grad_(x_grad)
            out = mc(xi)
            loss = (out * cot).sum()

            def run():
                loss.backward(retain_graph=True)
            return run

        fns = {"x.requires_grad": backward(True), "x frozen": backward(False)}
        res = alternate(fns, 5)
        say("  backward, %-6s   with x.requires_grad %7.3f ms   without %7.3f ms   (+%.3f ms, x%.2f)" % (
            arithmetic, res["x.requires_grad"], res["x frozen"], res["x.requires_grad"] - res["x frozen"], res["x.requires_grad"] / res["x frozen"]))
    with open(out_path, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
