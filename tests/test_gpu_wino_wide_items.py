"""The split-bf16 Winograd kernel's 64-output-channel work items (wino32b_kernel<2, ..>): every V fragment feeds the MFMAs of both
32-channel halves.  Each accumulator sums the same products in the same order as on 32-channel items, so the two forms must agree
BIT FOR BIT.  DCAP_WINO_COUT (read once per process) forces one form, so each form runs in a child process of its own."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import np_oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# N, H, W, Cin, Cout
BENCH_SHAPES = [(n, h, h, c, c) for n in (1, 2) for (h, c) in ((256, 64), (128, 128), (64, 256), (32, 512))] + \
               [(n, h, h, 256, 256) for n in (1, 2) for h in (256, 128, 64, 32)]         # stages 2-5, fpn_p2-p5 of a 1024 x 1024 input
RAGGED_SHAPES = [
    (1, 9, 7, 64, 128),          # odd H and W: half-empty edge tiles, one item per channel slice
    (2, 33, 17, 32, 96),         # Cout = 96: 32-channel items whatever is forced; Cin = 32: one K pair
    (1, 21, 45, 32, 64),         # Cin = 32 on 64-channel items
    (3, 104, 88, 160, 192),      # 7 x 6 groups x 3 images x 3 slices: blocks walk 1 and 2 items, odd KP = 5
    (1, 71, 119, 96, 288),       # Cout = 288: 32-channel items
]

_CHILD = r"""
import sys, torch
from image_captioning_amd import ops
shapes, path = eval(sys.argv[1]), sys.argv[2]
outs = []
for (N, H, W, Cin, Cout) in shapes:
    g = torch.Generator(device='cuda').manual_seed(N * 1000003 + H * 1009 + W * 7 + Cin * 31 + Cout)
    x = torch.randn(N, H, W, Cin, device='cuda', generator=g)
    w = torch.randn(Cout, 9 * Cin, device='cuda', generator=g) / (9 * Cin) ** 0.5
    sc = torch.rand(Cout, device='cuda', generator=g) + 0.5
    sh = torch.randn(Cout, device='cuda', generator=g)
    u = ops.winograd_pack_b3(w, Cin, Cout)
    args = (x, w, 3, 3, 1, 1, 1, H, W, sc, sh, None, 0, True)
    assert ops.conv2d_kernel_name(*args, w_wino_b3=u) == 'wino32b_kernel'
    out = torch.full((N, H, W, Cout), float('nan'), device='cuda')
    outs.append(ops.conv2d(*args, out=out, w_wino_b3=u).cpu())
torch.cuda.synchronize()
torch.save(outs, path)
"""


def _run(shapes, cout, path):
    env = dict(os.environ, DCAP_WINO_COUT=str(cout))
    r = subprocess.run([sys.executable, "-c", _CHILD, repr(shapes), str(path)], env=env, cwd=ROOT, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    return torch.load(str(path))


@pytest.mark.parametrize("shapes", [BENCH_SHAPES, RAGGED_SHAPES], ids=["benchmark", "ragged"])
def test_wide_items_bit_identical_to_32_channel_items(tmp_path, shapes):
    narrow = _run(shapes, 32, tmp_path / "narrow.pt")
    wide = _run(shapes, 64, tmp_path / "wide.pt")
    for s, a, b in zip(shapes, narrow, wide):
        assert bool(torch.isfinite(a).all()), s
        assert torch.equal(a, b), "%s: max |diff| %.3e" % (s, float((a - b).abs().max()))


@pytest.mark.parametrize("case", [(2, 64, 64, 256, 256), (1, 71, 57, 64, 128)])
def test_wide_items_against_float64_at_item_seams(tmp_path, case):
    """64-channel items against the float64 oracle on windows across the 8 x 16-pixel item seams, the image edges and the image seam,
    over all output channels (both halves of every sampled item)."""
    N, H, W, Cin, Cout = case
    got = _run([case], 64, tmp_path / "wide.pt")[0].numpy().astype(np.float64)
    g = torch.Generator(device="cuda").manual_seed(N * 1000003 + H * 1009 + W * 7 + Cin * 31 + Cout)
    x = torch.randn(N, H, W, Cin, device="cuda", generator=g)
    w = torch.randn(Cout, 9 * Cin, device="cuda", generator=g) / (9 * Cin) ** 0.5
    sc = torch.rand(Cout, device="cuda", generator=g) + 0.5
    sh = torch.randn(Cout, device="cuda", generator=g)
    xh = x.cpu().numpy().astype(np.float64)
    wk = w.cpu().numpy().astype(np.float64).reshape(Cout, 3, 3, Cin).transpose(1, 2, 3, 0)     # HWIO
    sch, shh = sc.cpu().numpy().astype(np.float64), sh.cpu().numpy().astype(np.float64)
    scale = max(1.0, float(np.abs(got).max()))
    S = 12
    ys = sorted({0, H - S, max(0, 8 - S // 2), max(0, (H // 16) * 8 - S // 2), max(0, H - 8 - S // 2)})
    xs = sorted({0, W - S, max(0, 16 - S // 2), max(0, (W // 32) * 16 - S // 2), max(0, W - 16 - S // 2)})
    worst = 0.0
    for n in sorted({0, N - 1}):
        for y0 in ys:
            for x0 in xs:
                y1, x1 = min(H, y0 + S), min(W, x0 + S)
                patch = np.zeros((1, y1 - y0 + 2, x1 - x0 + 2, Cin))
                sy0, sx0, sy1, sx1 = max(0, y0 - 1), max(0, x0 - 1), min(H, y1 + 1), min(W, x1 + 1)
                patch[0, sy0 - (y0 - 1):sy1 - (y0 - 1), sx0 - (x0 - 1):sx1 - (x0 - 1)] = xh[n, sy0:sy1, sx0:sx1]
                want = np.maximum(O.conv2d_nhwc(patch, wk, None, 1, 'valid')[0] * sch + shh, 0)
                worst = max(worst, float(np.abs(got[n, y0:y1, x0:x1] - want).max()))
    assert worst / scale < 2e-5, "windows vs float64 oracle: %.3e" % (worst / scale)
