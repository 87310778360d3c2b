"""K29 (aesmc_affine_quadratic_logweight_backward) and K30 (aesmc_adapted_draw_backward, alone and followed by the sorted
gather backward that makes the location's gradient of its h) beside the same adjoints composed from PyTorch operations on
the same device — float64 matmul / einsum for the chains and the sums, index_add_ for the gather's backward.  Everything
is timed warm between HIP events around runs of back-to-back calls (the host's share of a single call would otherwise
be measured with it), the runs alternating within each repetition; the median per call is reported with the spread, each
kernel beside its algorithmic bytes and the fraction of the HBM peak they make.
    python tools/bench_adapted_backward.py [B,K,D,Dy ...]        (default: 1024,4096,10,10; float32 particles)"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import aesmc_amd  # noqa: E402,F401
from aesmc_amd import _kernels  # noqa: E402

dev = torch.device("cuda", 0)
k = _kernels.get()
PEAK_HBM = 8000e9      # MI355X, bytes/s


def timed(fns, warm, reps, run=8):
    """Median, min and max in microseconds per call of every callable of `fns`: `run` back-to-back calls between two
    events (the first call's launch overlaps nothing, the others queue behind it), the runs taken in turn."""
    for _ in range(warm):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(reps):
        for fn, record in zip(fns, times):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            fn()
            a.record()
            for _ in range(run):
                fn()
            b.record()
            torch.cuda.synchronize()
            record.append(a.elapsed_time(b) * 1e3 / run)
    return [(sorted(t)[len(t) // 2], min(t), max(t)) for t in times]


def quadratic_composition(loc, P, o, g):
    wide = loc.double()
    w = -g.double().unsqueeze(-1) * (wide @ P.t() + o.unsqueeze(1))
    return (w @ P).to(loc.dtype), torch.einsum("bkj,bki->ji", w, wide), w.sum(dim=1)


def draw_composition(loc, idx, M, eps, G, flat):
    """(the location's gradient, grad_M, grad_L, grad_r): the gather's backward is index_add_ over the flattened rows."""
    B, K, D = loc.shape
    wide = G.double()
    moved = torch.gather(loc, 1, idx.unsqueeze(-1).expand(-1, -1, D)).double()
    h = (wide @ M).to(loc.dtype)
    grad_loc = torch.zeros(B * K, D, dtype=loc.dtype, device=loc.device).index_add_(0, flat, h.reshape(B * K, D))
    return (grad_loc.view(B, K, D), torch.einsum("bkj,bki->ji", wide, moved),
            torch.tril(torch.einsum("bkj,bki->ji", wide, eps.double())), wide.sum(dim=1))


print("tools/bench_adapted_backward.py on one {} ({}), float32 particles, HIP events, warm; us per call: median (min .. "
      "max); bytes by the algorithm; fraction of the {:.0f} GB/s HBM peak".format(
          torch.cuda.get_device_name(0), k._lib.aesmc_target_arch().decode(), PEAK_HBM / 1e9))
for spec in sys.argv[1:] or ["1024,4096,10,10"]:
    B, K, D, Dy = [int(v) for v in spec.split(",")]
    gen = torch.Generator(device=dev).manual_seed(0)
    rand = lambda *shape, dtype=torch.float32: torch.randn(*shape, device=dev, generator=gen, dtype=dtype)
    loc, eps, G, g = rand(B, K, D), rand(B, K, D), rand(B, K, D), rand(B, K)
    P, M, o = rand(Dy, D, dtype=torch.float64), rand(D, D, dtype=torch.float64), rand(B, Dy, dtype=torch.float64)
    # ancestors as a resampling step leaves them: sorted, about 60 % of the particles survive
    idx = torch.sort(torch.randint(0, K, (B, K), device=dev, generator=gen), dim=1).values
    flat = (idx + K * torch.arange(B, device=dev).unsqueeze(1)).reshape(-1)
    N, esz = B * K, 4
    survivors = int((idx[:, 1:] != idx[:, :-1]).sum().item()) + B
    bytes_29 = N * esz * (2 * D + 1) + 128 * (N // 64)
    bytes_30 = N * (esz * 3 * D + 8) + survivors * D * esz + 128 * (N // 64)
    bytes_gather = N * (8 + 2 * D * esz)
    calls = [
        ("K29 (grad_loc, grad_P, grad_offset)", bytes_29, lambda: k.affine_quadratic_logweight_backward(loc, P, o, g)),
        ("K29 without grad_loc", bytes_29 - N * D * esz,
         lambda: k.affine_quadratic_logweight_backward(loc, P, o, g, need_loc=False)),
        ("K30 (h, grad_M, grad_L, grad_r)", bytes_30, lambda: k.adapted_draw_backward(loc, idx, M, M, eps, G)),
        ("K30 without h", bytes_30 - N * D * esz, lambda: k.adapted_draw_backward(loc, idx, M, M, eps, G, need_h=False)),
        ("K30 + the sorted gather backward", bytes_30 + bytes_gather,
         lambda: k.gather_backward(k.adapted_draw_backward(loc, idx, M, M, eps, G)[0], idx, sorted_index=True)),
        ("PyTorch composition of K29", None, lambda: quadratic_composition(loc, P, o, g)),
        ("PyTorch composition of K30 + index_add_", None, lambda: draw_composition(loc, idx, M, eps, G, flat)),
    ]
    mine, theirs = calls[0][2](), quadratic_composition(loc, P, o, g)
    for name, a, b in zip(("grad_loc", "grad_P", "grad_offset"), mine, theirs):
        print("  K29 {:11s} largest difference from the composition {:.1e} (largest magnitude {:.1e})".format(
            name, float((a.double() - b.double()).abs().max()), float(b.abs().max())))
    h, grad_M, grad_L, grad_r = calls[2][2]()
    theirs = draw_composition(loc, idx, M, eps, G, flat)
    for name, a, b in zip(("grad_loc", "grad_M", "grad_L", "grad_r"),
                          (k.gather_backward(h, idx, sorted_index=True), grad_M, grad_L, grad_r), theirs):
        print("  K30 {:11s} largest difference from the composition {:.1e} (largest magnitude {:.1e})".format(
            name, float((a.double() - b.double()).abs().max()), float(b.abs().max())))
    results = timed([fn for _, _, fn in calls[:5]], 3, 9) + timed([fn for _, _, fn in calls[5:]], 1, 3, run=2)
    print("B={} K={} D={} Dy={}: {} of {} ancestors distinct".format(B, K, D, Dy, survivors, N))
    for (name, nbytes, _), result in zip(calls, results):
        tail = "" if nbytes is None else "   {:7.1f} MB, {:.3f} of the peak".format(
            nbytes / 1e6, nbytes / (result[0] * 1e-6) / PEAK_HBM)
        print("  {:42s} {:9.1f} ({:.1f} .. {:.1f}) us{}".format(name, *result, tail))
    print("  composition / K29 = {:.2f}x;  composition / (K30 + gather backward) = {:.2f}x".format(
        results[5][0] / results[0][0], results[6][0] / results[4][0]), flush=True)
