"""The GroupNorm(+SiLU) apply pass (launch_groupnorm_apply) against a device copy of the same bytes.

Timing (default): every apply shape of the SD2.1 512^2 batch-32 CFG UNet step (64 image rows) and of the VAE decoder
at the chunk its forward() picks for that batch (11 images), graph-replayed; the median over the replays, with a bf16
``copy_`` of the same element count timed the same way in the same process.  Prints us and TB/s (read + write) of
both and their ratio.

``--hashes``: one SHA-256 per shape of the output for seeded inputs, with silu on and off, on small batches of the
same shapes plus odd ones.  Two builds that compute the same thing print the same listing.

python tools/bench_gn_apply.py [--hashes] [--only unet|vae] [--iters 16] [--reps 7]
"""
import argparse
import hashlib
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from shai_amd import ops  # noqa: E402

# (name, HW, C1, C2, silu, calls per UNet step); read off models/unet2d.py (block_out_channels 320/640/1280/1280,
# two ResNets per down block, three per up block whose norm1 reads the skip concat as two sources, transformer
# input norms without SiLU, conv_norm_out).  N = 64 rows (batch 32 x 2 guidance halves).
UNET = [
    ("64^2 320", 4096, 320, 0, True, 8),          # down0 norm1/2 x2, up3 norm2 x3, conv_norm_out
    # (the five transformer input norms at 64^2 are folded into proj_in, Transformer2D._proj_in_gn_folded: no pass)
    ("64^2 320+320", 4096, 320, 320, True, 2),    # up3 resnets 1, 2 norm1
    ("64^2 640+320", 4096, 640, 320, True, 1),    # up3 resnet 0 norm1
    ("32^2 320", 1024, 320, 0, True, 1),          # down1 resnet 0 norm1 (320 -> 640)
    ("32^2 640", 1024, 640, 0, True, 6),          # down1 rest, up2 norm2 x3
    ("32^2 640 nosilu", 1024, 640, 0, False, 5),  # transformer input norms, level 1
    ("32^2 640+320", 1024, 640, 320, True, 1),    # up2 resnet 2 norm1
    ("32^2 640+640", 1024, 640, 640, True, 1),    # up2 resnet 1 norm1
    ("32^2 1280+640", 1024, 1280, 640, True, 1),  # up2 resnet 0 norm1
    ("16^2 640", 256, 640, 0, True, 1),           # down2 resnet 0 norm1 (640 -> 1280)
    ("16^2 1280", 256, 1280, 0, True, 6),         # down2 rest, up1 norm2 x3
    ("16^2 1280 nosilu", 256, 1280, 0, False, 5),  # transformer input norms, level 2
    ("16^2 1280+640", 256, 1280, 640, True, 1),   # up1 resnet 2 norm1
    ("16^2 1280+1280", 256, 1280, 1280, True, 2),  # up1 resnets 0, 1 norm1
    ("8^2 1280", 64, 1280, 0, True, 11),          # down3 x4, mid x4, up0 norm2 x3
    ("8^2 1280 nosilu", 64, 1280, 0, False, 1),   # mid transformer input norm
    ("8^2 1280+1280", 64, 1280, 1280, True, 3),   # up0 norm1 x3
]  # 56 calls per step
# VAE decoder (block_out_channels 128/256/512/512, latent 64^2), single source; the mid attention's norm has no SiLU
VAE = [
    ("vae 64^2 512", 64 * 64, 512, 0, True, 1),
    ("vae 64^2 512 nosilu", 64 * 64, 512, 0, False, 1),
    ("vae 128^2 512", 128 * 128, 512, 0, True, 1),
    ("vae 256^2 512", 256 * 256, 512, 0, True, 1),
    ("vae 256^2 256", 256 * 256, 256, 0, True, 1),
    ("vae 512^2 256", 512 * 512, 256, 0, True, 1),
    ("vae 512^2 128", 512 * 512, 128, 0, True, 1),
]
UNET_ROWS, VAE_ROWS = 64, 11
# --hashes: (N, HW, C1, C2) -- the shapes above at 2-3 images, and sizes that are no multiple of anything
HASH_SHAPES = [(1, 1, 8, 0), (3, 5, 8, 8), (7, 3, 24, 16), (2, 37, 40, 0), (1, 4099, 320, 0), (5, 64, 1280, 0),
               (3, 64, 1280, 640), (3, 64, 1280, 1280), (2, 1000, 640, 320), (2, 4096, 320, 0), (2, 4096, 320, 320),
               (2, 4096, 640, 320), (3, 1024, 640, 640), (2, 1024, 1280, 640), (3, 256, 1280, 1280), (2, 256, 640, 0),
               (2, 16384, 512, 0), (1, 65536, 256, 0), (1, 262144, 128, 0), (1, 300, 4104, 0)]


def median_time(fn, iters, reps):
    """Seconds per call: `iters` calls captured into one HIP graph, the median over `reps` timed replays."""
    fn()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        fn()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            for _ in range(iters):
                fn()
    torch.cuda.synchronize()
    g.replay()  # warm-up replay
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / iters * 1e-3)
    return statistics.median(ts)


def inputs(n, hw, c1, c2, seed):
    """Seeded on the host, so two builds see the same bits."""
    g = torch.Generator().manual_seed(seed)
    c = c1 + c2
    x = (torch.randn(n, hw, c1, generator=g) * 2.0 + 0.5).bfloat16().cuda()
    x2 = (torch.randn(n, hw, c2, generator=g) - 0.25).bfloat16().cuda() if c2 else None
    sc = (torch.randn(n, c, generator=g) * 0.5 + 1.0).cuda()
    sh = (torch.randn(n, c, generator=g) * 0.5).cuda()
    return x, x2, sc, sh


def device_inputs(n, hw, c1, c2):
    c = c1 + c2
    x = torch.randn(n, hw, c1, device="cuda").bfloat16()
    x2 = torch.randn(n, hw, c2, device="cuda").bfloat16() if c2 else None
    sc = torch.randn(n, c, device="cuda") * 0.5 + 1.0
    sh = torch.randn(n, c, device="cuda") * 0.5
    return x, x2, sc, sh


def timing(which, iters, reps):
    K = ops._K()
    rows = ([(UNET_ROWS,) + s for s in UNET] if which in ("all", "unet") else []) + \
           ([(VAE_ROWS,) + s for s in VAE] if which in ("all", "vae") else [])
    print(f"{'shape':24s} {'N':>3s} {'MB r+w':>8s} {'apply us':>9s} {'TB/s':>6s} {'copy us':>9s} {'TB/s':>6s} {'apply/copy':>10s}")
    step_us = 0.0
    for n, name, hw, c1, c2, silu, calls in rows:
        x, x2, sc, sh = device_inputs(n, hw, c1, c2)
        c = c1 + c2
        out = torch.empty(n, hw, c, dtype=torch.bfloat16, device="cuda")
        src = torch.randn(n * hw * c, device="cuda").bfloat16()
        dst = torch.empty_like(src)
        it = max(2, min(iters, int(2e9 // (4 * out.numel()))))  # ~1 GB of traffic per replay at least at the top
        ta = median_time(lambda: K.groupnorm_apply(x, x2, sc, sh, out, silu), it, reps)
        tc = median_time(lambda: dst.copy_(src), it, reps)
        nbytes = 4 * out.numel()
        print(f"{name:24s} {n:3d} {nbytes / 1e6:8.1f} {ta * 1e6:9.1f} {nbytes / ta / 1e12:6.2f} {tc * 1e6:9.1f} "
              f"{nbytes / tc / 1e12:6.2f} {tc / ta:10.2f}", flush=True)
        if n == UNET_ROWS:
            step_us += ta * 1e6 * calls
        del x, x2, out, src, dst
    if which in ("all", "unet"):
        print(f"apply passes of one batch-32 UNet step, calls x median: {step_us / 1e3:.3f} ms", flush=True)


def hashes():
    K = ops._K()
    for i, (n, hw, c1, c2) in enumerate(HASH_SHAPES):
        x, x2, sc, sh = inputs(n, hw, c1, c2, 1000 + i)
        for silu in (True, False):
            out = torch.empty(n, hw, c1 + c2, dtype=torch.bfloat16, device="cuda")
            K.groupnorm_apply(x, x2, sc, sh, out, silu)
            h = hashlib.sha256(out.view(torch.int16).cpu().numpy().tobytes()).hexdigest()
            print(f"{n}x{hw}x{c1}+{c2} silu={int(silu)} {h}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hashes", action="store_true")
    ap.add_argument("--only", choices=["all", "unet", "vae"], default="all")
    ap.add_argument("--iters", type=int, default=16)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    with torch.inference_mode():
        if a.hashes:
            hashes()
        else:
            timing(a.only, a.iters, a.reps)


if __name__ == "__main__":
    main()
