"""`tests.collapsed_provider.CollapsedOracle` plus the two backward calls of the differentiable collapsed-mixture evidence,
answered by the NumPy contracts of K52 / K53 and K54 (aesmc_amd/testing/switching_collapsed_backward.py), with a record of
what each call was asked for."""
import torch

from aesmc_amd.testing import switching_collapsed_backward as backward
from tests.collapsed_provider import CollapsedOracle

GRADIENTS = ("m0", "s0", "A", "b", "q", "C", "d", "r")


class CollapsedBackwardOracle(CollapsedOracle):
    def __init__(self):
        super().__init__()
        self.asked = []

    def switching_kalman_step_backward(self, model, regime, state, observation, grad_mean, grad_cov, grad_log_weight,
                                       observed=None, need_state=True, need=GRADIENTS):
        later = state is not None
        need = tuple(name for name in GRADIENTS if name in need and not (later and name in ("m0", "s0")))
        need_mean, need_cov = need_state if isinstance(need_state, (tuple, list)) else (need_state, need_state)
        need_mean, need_cov = bool(need_mean) and later, bool(need_cov) and later
        need_state = need_mean or need_cov
        assert need or need_state
        self.asked.append(("kalman" if later else "kalman0", need_state, need, observed is not None))
        ops = {name: value.detach().numpy() for name, value in model.items()}
        parts = None if state is None else tuple(part.detach().numpy() for part in state)
        out, flags = backward.switching_kalman_step_backward(
            ops, regime.numpy(), parts, observation.numpy(), grad_mean.numpy(), grad_cov.numpy(), grad_log_weight.numpy(),
            observed=None if observed is None else observed.numpy())
        self._flags |= flags
        grads = {name: torch.from_numpy(out["grad_" + name]) for name in need}
        return (torch.from_numpy(out["grad_mean_in"]) if need_mean else None,
                torch.from_numpy(out["grad_cov_in"]) if need_cov else None, grads)

    def switching_collapse_backward(self, means, covs, log_weights, grad_log_mass, grad_mean, grad_cov, need_means=True,
                                    need_covs=True, need_log_weights=True):
        assert need_means or need_covs or need_log_weights
        self.asked.append(("collapse", "shared" if means.dim() == 3 else "dense", need_means, need_covs, need_log_weights))
        grad_lw, grad_m, grad_P = backward.switching_collapse_backward(
            means.detach().numpy(), covs.detach().numpy(), log_weights.detach().numpy(), grad_log_mass.numpy(),
            grad_mean.numpy(), grad_cov.numpy())
        return (torch.from_numpy(grad_m) if need_means else None, torch.from_numpy(grad_P) if need_covs else None,
                torch.from_numpy(grad_lw) if need_log_weights else None)
