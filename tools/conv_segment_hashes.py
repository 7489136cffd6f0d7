"""Bit-equality listing for the v4 implicit-GEMM conv (csrc/kernels/gemm_8ph.hip, configs 9-12).

The conv's staging keeps a running source offset per DMA piece and recomputes the im2col address only when the
K position enters a new (filter tap, source tensor) segment.  The cases below are the smallest shapes at which that
state can go wrong: a tap change on every K-tile, split-K starting mid-tap, a concat with unequal halves, stride 2,
the two upsample forms, persistent workgroups that walk more than one tile, and the fat epilogue.

    python tools/conv_segment_hashes.py            # every config x split setting in child processes: the listing
    python tools/conv_segment_hashes.py --sd       # ... plus the three SD2.1 levels (batch 2, with / without concat)
    python tools/conv_segment_hashes.py --child [--check] [--sd]
        # this process only (SHAI_GEMM_FORCE / SHAI_GEMM_FORCE_SPLITS are read once per process); --check also
        # compares every output with the fp32 reference and exits non-zero on a miss

One line per output tensor: ``cfg splits case tensor sha256``.  Inputs are seeded per case on the CPU generator, so
two builds of the library print identical listings exactly when they compute identical bits.
"""
import argparse
import hashlib
import math
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CFGS = (9, 10, 11, 12)
SPLITS = (1, 3, 4)  # forced split-K counts (the host clamps them to the problem's maximum)

# (name, N, H, W, Cin, Cin2, Cout, k, stride, pad, kind, extras)
#   kind: "conv" plain, "up" nearest-2x upsample + 3x3 (9 taps, CONV 2), "up2" the same by output phase (CONV 3)
#   extras: any of "temb", "res", "gn", "silu"
CASES = [
    ("tap_per_tile", 5, 8, 8, 64, 0, 64, 3, 1, 1, "conv", ()),
    ("two_tiles_per_tap", 2, 16, 16, 128, 0, 320, 3, 1, 1, "conv", ()),
    ("concat_unequal", 2, 16, 16, 64, 128, 64, 3, 1, 1, "conv", ()),
    ("stride2_tails", 3, 12, 12, 128, 0, 96, 3, 2, 1, "conv", ()),
    ("one_by_one_concat", 2, 16, 16, 64, 64, 64, 1, 1, 0, "conv", ()),
    ("phase_temb_silu_gn", 2, 16, 16, 128, 0, 64, 3, 1, 1, "up2", ("temb", "silu", "gn")),
    ("phase_image_groups", 4, 8, 8, 64, 0, 64, 3, 1, 1, "up2", ("gn",)),
    # 20 K-tiles, 5 per tap: forced splits 3 start at tiles 7 and 14, inside a tap
    ("phase_split_mid_tap", 1, 16, 16, 320, 0, 64, 3, 1, 1, "up2", ("silu",)),
    ("upsample_nine_taps", 2, 8, 8, 128, 0, 64, 3, 1, 1, "up", ()),
    ("two_tiles_per_workgroup", 17, 64, 64, 64, 0, 64, 3, 1, 1, "conv", ()),
    ("fat_epilogue", 2, 16, 16, 128, 0, 320, 3, 1, 1, "conv", ("temb", "res", "gn")),
]
SD_CASES = [
    ("sd_320", 2, 64, 64, 320, 0, 320, 3, 1, 1, "conv", ()),
    ("sd_320_concat", 2, 64, 64, 320, 320, 320, 3, 1, 1, "conv", ()),
    ("sd_640", 2, 32, 32, 640, 0, 640, 3, 1, 1, "conv", ()),
    ("sd_640_concat", 2, 32, 32, 640, 640, 640, 3, 1, 1, "conv", ()),
    ("sd_1280", 2, 16, 16, 1280, 0, 1280, 3, 1, 1, "conv", ()),
    ("sd_1280_concat", 2, 16, 16, 1280, 1280, 1280, 3, 1, 1, "conv", ()),
]
TOL = {"conv": 2e-2, "up": 2e-2, "up2": 1e-2}  # relative Frobenius error against the fp32 reference


def _sha(t):
    import torch
    return hashlib.sha256(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()


def run_case(case, idx, check):
    """Run one case on the GPU.  Returns ([(tensor name, sha256)], [failure strings])."""
    import torch
    from shai_amd import ops
    from shai_amd.ops import reference as ref

    name, N, H, W, C, C2, Co, k, stride, pad, kind, extras = case
    g = torch.Generator().manual_seed(1000 + idx)
    rn = lambda *s: torch.randn(*s, generator=g).bfloat16()  # noqa: E731
    cin = C + C2
    x, x2 = rn(N, H, W, C), (rn(N, H, W, C2) if C2 else None)
    w = ops.pack_conv_weight((torch.randn(Co, cin, k, k, generator=g) / math.sqrt(cin * k * k)).bfloat16())
    b = rn(Co)
    up = kind != "conv"
    OH = ((2 * H if up else H) + 2 * pad - k) // stride + 1
    OW = ((2 * W if up else W) + 2 * pad - k) // stride + 1
    temb = rn(N, Co) if "temb" in extras else None
    res = rn(N, OH, OW, Co) if "res" in extras else None
    act = "silu" if "silu" in extras else None
    stats = "gn" if "gn" in extras else None
    dev = lambda t: None if t is None else t.cuda()  # noqa: E731
    kw = {}
    fails = []
    if kind == "up2":
        if not ops.up2_phases_ok(dev(x), k, k, stride, pad, temb=dev(temb)):
            fails.append(f"{name}: up2_phases_ok is false")
        kw["w_up2"] = ops.pack_up2_phase_weight(dev(w), C)
    y = ops.conv2d(dev(x), dev(w), dev(b), k, k, stride, pad, upsample=up, x2=dev(x2), temb=dev(temb),
                   residual=dev(res), act=act, stats=stats, **kw)
    gp = None
    if stats is not None:
        y, gp = y
        if gp is None:
            fails.append(f"{name}: no GroupNorm partials returned")
    torch.cuda.synchronize()
    hashes = [("out", _sha(y))]
    if gp is not None:
        hashes.append(("gn_partials", _sha(gp)))
    if check:
        yr = ref.conv2d(x, w, b, k, k, stride, pad, upsample=up, x2=x2, temb=temb, residual=res, act=act)
        rel = ((y.float().cpu() - yr.float()).norm() / yr.float().norm()).item()
        print(f"# {name}: rel {rel:.3e} (< {TOL[kind]:g})", flush=True)
        if not rel < TOL[kind]:
            fails.append(f"{name}: relative error {rel:.3e} >= {TOL[kind]:g}")
        if gp is not None:  # partials of the stored bf16 output, summed per image (as test_up2_phase_conv_forced)
            want = ref.col_partials(y.reshape(-1, Co)).reshape(N, -1, Co, 2).sum(1)
            try:
                torch.testing.assert_close(gp.reshape(N, -1, Co, 2).sum(1), want, atol=2e-1, rtol=1e-3)
            except AssertionError as e:
                fails.append(f"{name}: GroupNorm partials: {str(e)[:400]}")
    return hashes, fails


def child(check, sd):
    cfg = os.environ.get("SHAI_GEMM_FORCE", "-")
    splits = os.environ.get("SHAI_GEMM_FORCE_SPLITS", "1")
    fails = []
    for idx, case in enumerate(CASES + (SD_CASES if sd else [])):
        hashes, f = run_case(case, idx, check)
        fails += f
        for tname, h in hashes:
            print(f"cfg={cfg} splits={splits} {case[0]} {tname} {h}", flush=True)
    for f in fails:
        print("FAIL", f, flush=True)
    return 1 if fails else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--sd", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a.check, a.sd)
    rc = 0
    for cfg in CFGS:
        for sp in SPLITS:
            env = dict(os.environ, SHAI_GEMM_FORCE=str(cfg), SHAI_GEMM_FORCE_SPLITS=str(sp))
            cmd = [sys.executable, os.path.abspath(__file__), "--child"] + (["--check"] if a.check else []) + (
                ["--sd"] if a.sd else [])
            r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
            sys.stdout.write(r.stdout)
            sys.stdout.flush()
            if r.returncode != 0:
                sys.stderr.write(r.stderr[-3000:])
                return r.returncode  # a faulted or failed child: start nothing more on the GPU
    return rc


if __name__ == "__main__":
    sys.exit(main())
