"""The two launches of a fully adapted auxiliary particle filter step (aesmc_affine_quadratic_logweight, K27, and
aesmc_adapted_draw, K28) beside the composition of older launches that produces the same two outputs:

    first stage   K8 (r = P mu + o), then the elementwise work  base - 1/2 sum_j r_j^2
    draw          the gather (K3) of mu through the ancestors, K8 on the gathered rows (M mu[a] + r), K8 on the noise
                  (L eps), and the elementwise sum

Both are timed warm between HIP events around a run of launches issued back to back (one synchronisation per run), the
two alternating; the median over the runs is reported per launch (per composition) with the spread, the bytes a launch
moves by its algorithm, and that traffic as a fraction of the HBM peak bench.py prices against.  Behind them the measured
variance of log Z-hat of the adapted filter against `infer("smc")` with the transition as proposal, in the setting of
tests/test_gpu_adapted_filter.py.
    python tools/adapted_filter_bench.py [--out FILE] [B,K,D,Dy ...]
    (default: 1024,4096,10,10; float32; FILE defaults to profiles/adapted_filter.txt)"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import aesmc_amd  # noqa: E402,F401
from aesmc_amd import _kernels, adapted, inference  # noqa: E402
from aesmc_amd.testing import adapted as contract  # noqa: E402
from aesmc_amd.testing.models import LgssmNd  # noqa: E402

HBM_PEAK_GBPS = 8000.0      # bench.py's
dev = torch.device("cuda", 0)
k = _kernels.get()


def run_of(fn, launches):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / launches


def beside(kernel, composition, launches=50, runs=7):
    run_of(kernel, 10), run_of(composition, 3)
    times_k, times_c = [], []
    for _ in range(runs):
        times_k.append(run_of(kernel, launches))
        times_c.append(run_of(composition, max(3, launches // 4)))
    times_k.sort(), times_c.sort()
    return times_k, times_c


def variance_lines():
    lines = ["variance of log Z-hat over 512 replicas of one observation sequence, LgssmNd(2), T = 5, K = 64: adapted filter "
             "over infer('smc') with the transition as proposal"]
    for dtype in (torch.float32, torch.float64):
        model = LgssmNd(2, dtype=dtype, affine=True).to(dev)
        observations = [y.expand(512, 2).contiguous() for y in model.simulate(5, 1, seed=1)]
        torch.manual_seed(21)
        np.random.seed(21)
        mine = adapted.adapted_filter(observations, model.initial, model.transition, model.emission, 64)

        def proposal(previous_latents=None, time=None, observations=None):
            return model.initial() if time == 0 else model.transition(previous_latents=previous_latents, time=time)

        with torch.no_grad():
            boot = inference.infer("smc", observations, model.initial, model.transition, model.emission, proposal, 64,
                                   return_log_marginal_likelihood=True, return_latents=False, return_log_weight=False)
        a = mine["log_marginal_likelihood"].double().var().item()
        b = boot["log_marginal_likelihood"].double().var().item()
        lines.append("  {}: adapted {:.3e}, bootstrap {:.3e}, ratio {:.4f}".format(str(dtype)[6:], a, b, a / b))
    return lines


def main(argv):
    out_path = os.path.join(ROOT, "profiles", "adapted_filter.txt")
    if argv[:1] == ["--out"]:
        out_path, argv = argv[1], argv[2:]
    lines = ["K27 (aesmc_affine_quadratic_logweight) and K28 (aesmc_adapted_draw) beside the composition of K8, the gather and",
             "elementwise launches that gives the same outputs; float32 particles, one MI355X; us per call: median (min .. max)",
             "over runs of back-to-back launches between HIP events, the two alternating; bytes by the algorithm; fraction of",
             "the {:.0f} GB/s HBM peak".format(HBM_PEAK_GBPS)]
    for spec in argv or ["1024,4096,10,10"]:
        B, K, D, Dy = [int(v) for v in spec.split(",")]
        gen = torch.Generator(device=dev).manual_seed(0)
        rng = np.random.RandomState(0)
        gain = contract.gains(1.0, np.eye(Dy, D) + 0.01 * rng.randn(Dy, D), 0.5)
        o, r = contract.row_offsets(gain, rng.randn(B, Dy))
        f64 = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        P, M, L, o, r = f64(gain["P"]), f64(gain["M"]), f64(gain["L"]), f64(o), f64(r)
        P32, M32, L32, o32, r32 = P.float(), M.float(), L.float(), o.float(), r.float()
        mu = torch.randn(B, K, D, device=dev, generator=gen)
        eps = torch.randn(B, K, D, device=dev, generator=gen)
        idx = torch.sort(torch.randint(0, K, (B, K), device=dev, generator=gen), dim=1).values
        base = gain["base"]

        def first_stage():
            return k.affine_quadratic_logweight(mu, P, o, base)

        def first_stage_composed():
            residual = k.particle_affine(mu, P32, o32)
            return base - 0.5 * (residual * residual).sum(dim=2)

        def draw():
            return k.adapted_draw(mu, idx, M, r, L, eps)

        def draw_composed():
            return k.particle_affine(k.gather(mu, idx), M32, r32) + k.particle_affine(eps, L32)

        near = lambda a, b: float((a - b).abs().max())
        agree = (near(first_stage(), first_stage_composed()), near(draw(), draw_composed()))
        torch.cuda.synchronize()
        bytes_27 = B * K * 4 * (D + 1)
        bytes_28 = B * K * (8 + 4 * 3 * D)
        for name, kernel, composition, nbytes in (("K27", first_stage, first_stage_composed, bytes_27),
                                                  ("K28", draw, draw_composed, bytes_28)):
            tk, tc = beside(kernel, composition)
            mk, mc = tk[len(tk) // 2], tc[len(tc) // 2]
            lines.append("B={} K={} D={} Dy={}: {} {:.1f} ({:.1f} .. {:.1f}) us, {:.1f} MB, {:.3f} of the peak;  composition {:.1f} "
                         "({:.1f} .. {:.1f}) us;  composition / {} = {:.2f}x".format(
                             B, K, D, Dy, name, mk, tk[0], tk[-1], nbytes / 1e6, nbytes / (mk * 1e-6) / 1e9 / HBM_PEAK_GBPS,
                             mc, tc[0], tc[-1], name, mc / mk))
            print(lines[-1], flush=True)
        lines.append("  largest difference from the composition (float32 chains against float64 ones): K27 {:.2e}, K28 {:.2e}".format(
            *agree))
    lines += variance_lines()
    print("\n".join(lines[-4:]), flush=True)
    assert k.read_flags(dev) == 0
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as handle:
        handle.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
