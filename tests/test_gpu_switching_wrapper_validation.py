"""What the Python wrappers of the switching-model step and look-ahead kernels refuse before any launch, message by message,
and what they record for a launch they make: the C entry chosen, the name it is timed under and its algorithmic bytes.
M = 2, D = 2, Dy = 1, B = 2, K = 3 throughout; the byte counts are written out for these sizes."""
import pytest
import torch

pytestmark = pytest.mark.gpu

M, D, DY, B, K = 2, 2, 1, 2, 3
STEPS = ("switching_kalman_step", "switching_kalman_draw", "switching_kalman_conditional_step")
LOOKAHEADS = ("switching_lookahead", "switching_lookahead_scores")


def _provider():
    from aesmc_amd import _kernels
    provider = _kernels.get()
    assert provider.name == "hip"
    return provider


def _model(device, D=D, Dy=DY):
    f64 = dict(dtype=torch.float64, device=device)
    return {"cdf0": torch.tensor([0.5, 1.0], **f64), "cdf": torch.tensor([[0.75, 1.0], [0.25, 1.0]], **f64),
            "m0": torch.zeros(D, **f64), "s0": torch.ones(D, **f64), "A": (0.5 * torch.eye(D, **f64)).repeat(M, 1, 1),
            "b": torch.zeros(M, D, **f64), "q": torch.ones(M, D, **f64), "C": torch.ones(M, Dy, D, **f64),
            "d": torch.zeros(M, Dy, **f64), "r": torch.ones(M, Dy, **f64)}


def _state(device, D=D):
    TD = D * (D + 1) // 2
    cov = torch.zeros(B, K, TD, dtype=torch.float64, device=device)
    for i in range(D):
        cov[..., i * (i + 1) // 2 + i] = 1.0
    return (torch.zeros(B, K, dtype=torch.int32, device=device), torch.zeros(B, K, D, dtype=torch.float64, device=device), cov)


def _operands(device, name, later=True, masked=False, D=D, Dy=DY):
    """Valid keyword arguments of wrapper `name`."""
    given = dict(model=_model(device, D, Dy), state=_state(device, D) if later else None,
                 observation=torch.zeros(B, Dy, dtype=torch.float64, device=device),
                 observed=torch.ones(B, Dy, dtype=torch.bool, device=device) if masked else None)
    if name in STEPS:
        given.update(index=torch.arange(K, device=device).repeat(B, 1) if later else None,
                     uniforms=torch.full((B, K), 0.5, dtype=torch.float64, device=device))
        if name == "switching_kalman_draw":
            given["cdf"] = torch.tensor([0.5, 1.0], dtype=torch.float64, device=device).repeat(B, K, 1)
        if name == "switching_kalman_conditional_step":
            given["pinned_regime"] = torch.ones(B, dtype=torch.int32, device=device)
    else:
        given.update(log_prior=torch.full((M, M) if later else (M,), -0.6931471805599453, dtype=torch.float64, device=device),
                     num_particles=None if later else K)
    return given


def _refused(name, match, device, later=True, masked=False, D=D, Dy=DY, **changes):
    given = _operands(device, name, later, masked, D, Dy)
    for key, value in changes.items():
        given[key] = value(given[key]) if callable(value) else value
    with pytest.raises(ValueError, match=match):
        getattr(_provider(), name)(**given)


@pytest.mark.parametrize("name", STEPS + LOOKAHEADS)
def test_shared_refusals(hip_device, name):
    dev = hip_device
    step = name in STEPS
    _refused(name, r"observation must be \[2, 1\]" if step else r"observation must be \[batch_size, 1\]", dev,
             observation=torch.zeros(B, DY + 1, dtype=torch.float64, device=dev))
    if not step:
        _refused(name, r"observation must be \[batch_size, 1\]", dev, observation=torch.zeros(B, dtype=torch.float64, device=dev))
    for masked_observed in (torch.ones(B, DY, dtype=torch.uint8, device=dev), torch.ones(B, DY + 1, dtype=torch.bool, device=dev),
                            torch.ones(DY, dtype=torch.bool, device=dev)):
        _refused(name, r"observed must be None or a \[2, 1\] torch.bool tensor", dev, observed=masked_observed)
    for later in (False, True):
        _refused(name, r"b must be dense \(2, 2\) float64", dev, later=later,
                 model=lambda model: dict(model, b=torch.zeros(M, D + 1, dtype=torch.float64, device=dev)))
        _refused(name, r"cdf must be dense \(2, 2\) float64", dev, later=later,
                 model=lambda model: dict(model, cdf=model["cdf"].float()))
        # the refusal names the public method that was called
        _refused(name, "aesmc_amd: " + name + r" does not take these operands \(see switching_covers\)", dev, later=later, D=9)
        _refused(name, "aesmc_amd: " + name + r" does not take these operands \(see switching_covers\)", dev, later=later, Dy=9)
    _refused(name, r"regime must be \(2, 3\) torch.int32", dev, state=lambda s: (s[0].long(), s[1], s[2]))
    _refused(name, r"cov must be \(2, 3, 3\) torch.float64", dev, state=lambda s: (s[0], s[1], s[2][..., :2]))


@pytest.mark.parametrize("name", STEPS)
def test_step_refusals(hip_device, name):
    dev = hip_device
    for later in (False, True):
        _refused(name, r"regime uniforms must be \[batch_size, num_particles\] float64", dev, later=later,
                 uniforms=lambda u: u.float())
        _refused(name, r"regime uniforms must be \[batch_size, num_particles\] float64", dev, later=later,
                 uniforms=lambda u: u.reshape(-1))
    _refused(name, r"index must be \[2, 3\] int64", dev, index=lambda i: i.int())
    _refused(name, r"index must be \[2, 3\] int64", dev, index=lambda i: i[:, :2])
    if name == "switching_kalman_draw":
        for later in (False, True):
            _refused(name, r"cdf must be \(2, 3, 2\) float64", dev, later=later, cdf=lambda c: c[:, :, :1])
            _refused(name, r"cdf must be \(2, 3, 2\) float64", dev, later=later, cdf=lambda c: c.float())
    if name == "switching_kalman_conditional_step":
        for later in (False, True):
            _refused(name, r"pinned_regime must be \[2\] int32", dev, later=later, pinned_regime=lambda p: p.long())
            _refused(name, r"pinned_regime must be \[2\] int32", dev, later=later,
                     pinned_regime=torch.ones(B, K, dtype=torch.int32, device=dev))


@pytest.mark.parametrize("name", LOOKAHEADS)
def test_lookahead_refusals(hip_device, name):
    dev = hip_device
    half = -0.6931471805599453
    _refused(name, r"log_prior must be \(2, 2\) float64", dev, log_prior=torch.full((M,), half, dtype=torch.float64, device=dev))
    _refused(name, r"log_prior must be \(2,\) float64", dev, later=False,
             log_prior=torch.full((M, M), half, dtype=torch.float64, device=dev))
    _refused(name, r"log_prior must be \(2, 2\) float64", dev, log_prior=lambda p: p.float())
    _refused(name, "aesmc_amd: " + name + " without a state needs num_particles", dev, later=False, num_particles=None)
    _refused(name, "aesmc_amd: " + name + " without a state needs num_particles", dev, later=False, num_particles=-1)
    _refused(name, r"num_particles \(4\) disagrees with the state \(3\)", dev, num_particles=4)


# what a launch is recorded as: (C entry, timer name, bytes) by wrapper, (later, masked).  Bytes: 6 particles times the
# state read and written, the uniform, the index, the weight and the per-particle row; the observation's 2 x 8 bytes (and 2 of
# mask); the model's 224 bytes, 192 without the chain's rows (the draw)
RECORDED = {
    "switching_kalman_step": {
        (False, False): ("aesmc_switching_kalman_step", "switching_kalman_step", 6 * 60 + 16 + 224),
        (True, False): ("aesmc_switching_kalman_step", "switching_kalman_step", 6 * 112 + 16 + 224),
        (False, True): ("aesmc_switching_kalman_masked_step", "switching_kalman_masked_step", 6 * 60 + 18 + 224),
        (True, True): ("aesmc_switching_kalman_masked_step", "switching_kalman_masked_step", 6 * 112 + 18 + 224)},
    "switching_kalman_draw": {
        (False, False): ("aesmc_switching_kalman_draw", "switching_kalman_draw", 6 * 76 + 16 + 192),
        (True, False): ("aesmc_switching_kalman_draw", "switching_kalman_draw", 6 * 128 + 16 + 192),
        (False, True): ("aesmc_switching_kalman_masked_step", "switching_kalman_masked_draw", 6 * 76 + 18 + 192),
        (True, True): ("aesmc_switching_kalman_masked_step", "switching_kalman_masked_draw", 6 * 128 + 18 + 192)},
    "switching_kalman_conditional_step": {
        (False, False): ("aesmc_switching_kalman_conditional_step", "switching_kalman_conditional_step", 6 * 60 + 8 + 16 + 224),
        (True, False): ("aesmc_switching_kalman_conditional_step", "switching_kalman_conditional_step", 6 * 112 + 8 + 16 + 224),
        (False, True): ("aesmc_switching_kalman_masked_step", "switching_kalman_masked_conditional_step", 6 * 60 + 8 + 18 + 224),
        (True, True): ("aesmc_switching_kalman_masked_step", "switching_kalman_masked_conditional_step", 6 * 112 + 8 + 18 + 224)},
    "switching_lookahead": {
        (False, False): ("aesmc_switching_lookahead", "switching_lookahead", 6 * 24 + 16 + 224),
        (True, False): ("aesmc_switching_lookahead", "switching_lookahead", 6 * 68 + 16 + 224),
        (False, True): ("aesmc_switching_masked_lookahead", "switching_masked_lookahead", 6 * 24 + 18 + 224),
        (True, True): ("aesmc_switching_masked_lookahead", "switching_masked_lookahead", 6 * 68 + 18 + 224)},
    "switching_lookahead_scores": {
        (False, False): ("aesmc_switching_lookahead_scores", "switching_lookahead_scores", 6 * 24 + 16 + 224),
        (True, False): ("aesmc_switching_lookahead_scores", "switching_lookahead_scores", 6 * 68 + 16 + 224),
        (False, True): ("aesmc_switching_masked_lookahead_scores", "switching_masked_lookahead_scores", 6 * 24 + 18 + 224),
        (True, True): ("aesmc_switching_masked_lookahead_scores", "switching_masked_lookahead_scores", 6 * 68 + 18 + 224)},
}


@pytest.mark.parametrize("masked", (False, True))
@pytest.mark.parametrize("later", (False, True))
@pytest.mark.parametrize("name", STEPS + LOOKAHEADS)
def test_launch_is_recorded_under_its_name_and_bytes(hip_device, name, later, masked):
    from aesmc_amd import _kernels
    provider = _provider()
    given = _operands(hip_device, name, later, masked)
    timer = _kernels.KernelTimer()
    provider.timer = timer
    try:
        out = getattr(provider, name)(**given)
    finally:
        provider.timer = None
    assert provider.read_flags(hip_device) == 0
    entry, recorded_as, nbytes = RECORDED[name][later, masked]
    assert list(timer.launches) == [recorded_as]
    count, sample = timer.launches[recorded_as]
    assert count == 1 and sample[0][0][0].__name__ == entry and sample[0][1] == nbytes
    # the return order: the look-ahead gives (log_weight, cdf), its scores form (scores, log_weight); a step four tensors
    shapes = [tuple(t.shape) for t in out]
    if name == "switching_lookahead":
        assert shapes == [(B, K), (B, K, M)]
        assert torch.equal(out[1][..., -1], torch.ones(B, K, dtype=torch.float64, device=hip_device))      # a cumulative row
    elif name == "switching_lookahead_scores":
        assert shapes == [(B, K, M), (B, K)]
        assert torch.allclose(torch.logsumexp(out[0], dim=-1), out[1], rtol=0, atol=1e-12)
    else:
        assert shapes == [(B, K), (B, K, D), (B, K, D * (D + 1) // 2), (B, K)] and out[0].dtype == torch.int32
        if name == "switching_kalman_conditional_step":
            assert (out[0][:, K - 1] == 1).all()      # the pinned slot
        assert torch.isfinite(out[3]).all()
