"""The suite's oracle provider (tests/oracle_provider.py) plus what the collapsed-mixture filter and smoother call: K31
(under a mask: K39), K50 and K51 from their NumPy contracts, with a record of the calls."""
import torch

from aesmc_amd.testing import rao_blackwell as contract
from aesmc_amd.testing import switching_collapsed as collapsed
from aesmc_amd.testing import switching_missing as missing
from tests.oracle_provider import OracleKernels


class CollapsedOracle(OracleKernels):
    def __init__(self):
        super().__init__()
        self.calls, self.reads, self.masks = [], 0, []

    def read_flags(self, device):
        self.reads += 1
        return super().read_flags(device)

    def switching_limits(self):
        return 8, 8, 16

    def switching_covers(self, observation, num_regimes, latent_dim, observation_dim, num_particles):
        return torch.is_tensor(observation) and observation.dim() == 2 and observation.dtype in (torch.float32, torch.float64) \
            and observation.size(1) == observation_dim and latent_dim <= 8 and observation_dim <= 8 and num_regimes <= 16

    def switching_kalman_step(self, model, state, index, uniforms, observation, observed=None):
        assert index is None
        self.calls.append(("kalman0" if state is None else "kalman", uniforms.size(1)))
        self.masks.append(observed)
        ops = {name: value.numpy() for name, value in model.items()}
        parts = None if state is None else tuple(part.numpy() for part in state)
        args = (ops, parts, None, uniforms.numpy(), observation.numpy())
        regime, mean, cov, log_w, flags = contract.switching_kalman_step(*args) if observed is None else \
            missing.switching_kalman_step(*args, observed.numpy())
        self._flags |= flags
        return torch.from_numpy(regime), torch.from_numpy(mean), torch.from_numpy(cov), torch.from_numpy(log_w)

    def switching_collapse(self, means, covs, log_weights):
        self.calls.append(("collapse", "shared" if means.dim() == 3 else "dense") + tuple(log_weights.shape[1:]))
        assert log_weights.dim() == 3 and means.dim() == covs.dim() and means.dtype == covs.dtype == log_weights.dtype == torch.float64
        out = collapsed.switching_collapse(means.numpy(), covs.numpy(), log_weights.numpy())
        return tuple(torch.from_numpy(part) for part in out)

    def switching_pair_smooth(self, model, mean, cov, mean_next, cov_next):
        self.calls.append(("pair",))
        assert mean.shape == mean_next.shape and cov.shape == cov_next.shape and mean.dim() == 3
        ops = {name: value.numpy() for name, value in model.items()}
        means, covs, _ = collapsed.switching_pair_smooth(ops, mean.numpy(), cov.numpy(), mean_next.numpy(), cov_next.numpy())
        return torch.from_numpy(means), torch.from_numpy(covs)
