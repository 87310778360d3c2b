"""Host-side launcher for the HIP kernels: validates operands, allocates outputs, enqueues on the
caller's current HIP stream through the C ABI (include/aesmc_hip.h).

Every operand is checked here against what the kernel and its grid assume (device, dtype, shape,
density, alignment) before anything is launched.  Kernels report data-dependent conditions (NaN
log-weights, degenerate rows, out-of-range indices) by OR-ing bits into a per-device int32 word
that the host reads once per ELBO evaluation (`read_flags`) instead of synchronising per timestep.
"""
import contextlib
import ctypes
import threading

import torch

from . import _lib
from . import settings

_DTYPE_TAG = {torch.float32: _lib.F32, torch.float64: _lib.F64}


def _require_hip(t, what):
    if not isinstance(t, torch.Tensor):
        raise AttributeError("{} must be a torch.Tensor. Got: {}".format(what, type(t)))
    if not t.is_cuda:
        raise RuntimeError(
            "aesmc_amd: {} lives on '{}'; this package computes only on a HIP device (MI355X) "
            "and has no CPU fallback.".format(what, t.device))


def _tag(t, what):
    try:
        return _DTYPE_TAG[t.dtype]
    except KeyError:
        raise TypeError("aesmc_amd: {} must be float32 or float64, got {}".format(what, t.dtype))


def _inner_dense(t):
    """True when dims 2.. of `t` are laid out densely (row payload is one contiguous run)."""
    expect = 1
    for size, stride in zip(reversed(t.shape[2:]), reversed(t.stride()[2:])):
        if size != 1 and stride != expect:
            return False
        expect *= size
    return True


def _ptr(t):
    return 0 if t is None else t.data_ptr()


_NO_SWITCH = contextlib.nullcontext()
# torch.cuda.current_device() without its lazy-initialisation checks: a launch's operands already live on the device
_current_device = getattr(torch._C, "_cuda_getDevice", None) or torch.cuda.current_device
_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _on_device(device):
    """Context that makes `device` current for the launch; free when it already is (the usual
    case: entering torch.cuda.device costs ~4 us of host time per kernel in the eager loop)."""
    if _current_device() == device.index:
        return _NO_SWITCH
    return torch.cuda.device(device)


class PackedAncestors:
    """What a resampling step hands to the launches that consume its ancestry INSIDE the library, on the lean route of
    `infer` (`settings.packed_ancestors`): `words` int32 [B,K] holding aesmc_resample_step_packed's uint32 words — the
    ancestor index in the low half, where the particle's children end in the high half (`has_ranges`; else 0) — 4 bytes
    per particle where the int64 indices and int32 ranges are 12.  K16 and K14's rows form read the words as they are;
    everything else asks for `index()` / `child_end()`: ONE unpack launch (aesmc_unpack_ancestors), memoised — the int64
    [B,K] tensor `ancestor_index` would have returned (tagged sorted) and the int32 ranges.  Nothing else unpacks: the
    handle is not a tensor and forwards no tensor attributes.  Three explicit conveniences for a wrapper around the
    provider's `resample_step` that records or overrides a step's ancestors — `clone()` and `cpu()` (copies of the int64
    indices) and `copy_()` (the indices overwritten, the words following) — each an unpack, none used by the package."""
    __slots__ = ("words", "has_ranges", "_idx", "_ends", "_aesmc_sorted")

    def __init__(self, words, has_ranges):
        self.words, self.has_ranges = words, bool(has_ranges)
        self._idx = self._ends = None
        self._aesmc_sorted = True

    shape = property(lambda self: self.words.shape)
    device = property(lambda self: self.words.device)

    def index(self):
        if self._idx is None:
            self._idx, self._ends = get().unpack_ancestors(self.words, self.has_ranges)
            self._idx._aesmc_sorted = True
            if self._ends is not None:
                self._idx._aesmc_child_end = self._ends
        return self._idx

    def child_end(self):
        if not self.has_ranges:
            return None
        self.index()
        return self._ends

    def clone(self):
        return self.index().clone()

    def cpu(self):
        return self.index().cpu()

    def copy_(self, source):
        """`Tensor.copy_` on the int64 indices (non-decreasing along the particles, as every resampler's): the words
        follow, and the ranges — where each particle's children end — are formed again from the new indices."""
        idx = self.index()
        idx.copy_(source)
        wide = idx.clone()
        if self.has_ranges:
            B, K = idx.shape
            position = torch.arange(K, device=idx.device).unsqueeze(0).expand(B, K).contiguous()
            self._ends.copy_(torch.searchsorted(idx.contiguous(), position, right=True))
            wide |= self._ends.to(torch.int64) << 16
        self.words.copy_(torch.where(wide >= 2 ** 31, wide - 2 ** 32, wide))
        return self


def as_index(index):
    """The int64 ancestor indices behind `index`: a `PackedAncestors` unpacks (once), a tensor is returned as it is."""
    return index.index() if type(index) is PackedAncestors else index


class KernelTimer:
    """Optional per-kernel timing for bench.py's `roofline` leg.  While installed on the provider
    it keeps a bounded random sample of the launches made (the C-ABI entry point with its operands);
    `summary()` then captures each kernel's sample, launched back to back, into one hipGraph and
    times replays of it between two HIP events on the replaying stream: kernel time on the real
    operands without host gaps (a 9 us kernel cannot be timed through ~10 us Python launches).  The
    sample cycles through distinct operands, so caches are as cold as in the workload.  `bytes` is
    the ALGORITHMIC traffic of a launch: what the operation must move, not
    what the hardware happened to move."""

    def __init__(self, keep=24, seed=0):
        import random
        self.keep = keep
        self.random = random.Random(seed)
        self.launches = {}   # name -> [count, [(fn, nbytes, keepalive), ...]]

    def note(self, name, fn, nbytes, keepalive):
        """`fn` = (entry point, argument tuple whose LAST element is the stream)."""
        entry = self.launches.setdefault(name, [0, []])
        entry[0] += 1
        if len(entry[1]) < self.keep:
            entry[1].append((fn, nbytes, keepalive))
        else:  # reservoir sampling keeps a uniform sample of all launches seen
            slot = self.random.randrange(entry[0])
            if slot < self.keep:
                entry[1][slot] = (fn, nbytes, keepalive)

    def summary(self, repeats=3):
        provider = get()
        provider.timer = None       # the replays (and the K7 call below) must not be noted again
        out = {}
        for name, (count, sample) in list(self.launches.items()):
            def launch_all():
                stream = torch.cuda.current_stream().cuda_stream
                for (entry, args), _, _ in sample:
                    entry(*(args[:-1] + (stream,)))
            torch.cuda.synchronize()
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):      # warm-up off the default stream, as capture requires
                launch_all()
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            # thread_local: with a process group alive RCCL's watchdog thread may call the HIP runtime
            # at any time; that must not invalidate this capture
            with torch.cuda.graph(graph, capture_error_mode="thread_local"):
                launch_all()
            graph.replay()
            torch.cuda.synchronize()
            begin = torch.cuda.Event(enable_timing=True)
            end = torch.cuda.Event(enable_timing=True)
            begin.record()
            for _ in range(repeats):
                graph.replay()
            end.record()
            torch.cuda.synchronize()
            del graph
            seconds = begin.elapsed_time(end) * 1e-3 / (repeats * len(sample))
            nbytes = sum(n for _, n, _ in sample) / len(sample)
            out[name] = {"launches": count, "sampled": len(sample), "avg_us": 1e6 * seconds,
                         "bytes_per_launch": nbytes, "GBps": nbytes / seconds / 1e9}
            if name in ("resample_gather", "resample_step", "affine_normal_propagate_resampled",
                        "affine_normal_propagate_drawn"):
                # The algorithmic figure counts a full read of the source (and, for the fused step,
                # K3's re-read of the indices, which it skips); only rows that still have offspring
                # are actually fetched.  Report how many that was on these operands and the bytes
                # that had to move.
                fractions, moved, ess = [], [], []
                for _, _, keep in sample:
                    if name in ("affine_normal_propagate_resampled", "affine_normal_propagate_drawn"):
                        # (x_src, ancestors, eps, y, lw, x_t, ...): the gather's read side is the surviving rows
                        idx, dst = keep[1], keep[5]
                        if idx is None:
                            continue
                        if idx.dtype == torch.int32:      # the packed words: the index is the low half
                            idx = idx & 0xffff
                        rows = idx.numel()
                        unique = int((idx[:, 1:] != idx[:, :-1]).sum().item()) + idx.size(0)
                        payload = dst.numel() * dst.element_size() / rows
                        fractions.append(unique / rows)
                        noise_rows = 2 if name == "affine_normal_propagate_resampled" else 1     # eps read + x_t written
                        moved.append(rows * (8 + dst.element_size() + noise_rows * payload) + unique * payload)
                        continue
                    idx, dst = (keep[1], keep[2]) if name == "resample_gather" else (keep[2], keep[5])
                    if dst is None:
                        continue
                    if name == "resample_step":   # effective sample size of the weights resampled from (K7)
                        log_ess = get().particle_summary(keep[0], want_log_ess=True)[0]
                        ess.append(float(torch.exp(log_ess.double()).mean().item()) / idx.size(1))
                    rows = idx.numel()
                    unique = int((idx[:, 1:] != idx[:, :-1]).sum().item()) + idx.size(0)
                    payload = dst.numel() * dst.element_size() / rows
                    fractions.append(unique / rows)
                    fixed = rows * 8 if name == "resample_gather" else rows * (keep[0].element_size() + 8)
                    moved.append(fixed + (rows + unique) * payload)
                if fractions:
                    out[name]["unique_ancestor_fraction"] = sum(fractions) / len(fractions)
                    out[name]["moved_bytes_per_launch"] = sum(moved) / len(moved)
                    out[name]["moved_GBps"] = out[name]["moved_bytes_per_launch"] / seconds / 1e9
                if ess:
                    out[name]["ess_over_k"] = sum(ess) / len(ess)
        return out


class HipKernels:
    """The product backend.  One instance per process; per-device state is created lazily."""

    name = "hip"

    def __init__(self):
        self._lib = _lib.load()
        self._flags = {}
        self._lock = threading.Lock()
        self.timer = None  # set to a KernelTimer to time every launch (bench only)
        self._flag_constants = {}
        self.lds_max_particles = int(self._lib.aesmc_ancestor_index_lds_max_particles())
        self._affine_max_dim = None
        self._map_cache = {}        # id(weight) -> (weight, its aesmc_affine_map, (shape, strides))
        self._covers_last = None    # the operands of the last step `affine_logweight_covers` accepted
        self._wide_dim = None       # (aesmc_affine_wide_dim(), _min_dim(), _max_dim()): see `_wide_limits`
        self._pairs = None          # (key, tensor): the interleaved weight pairs of the maps the fused launch met last
        self.evaluation = 0         # bumped by `begin_evaluation`: what a cached weight-pair block belongs to
        self._statistics_workspaces = {}      # device index -> the two blocks of K45 / K46's partials
        self._statistics_sizes = {}           # (D, Dy, masked) -> a block's bytes; "limits": switching_limits(), read once
        self.WEIGHT_PAIRS = settings.knob("AESMC_K16_PAIRS", "1") != "0"      # measurement knob
        self.SCALED_PAIRS = settings.knob("AESMC_K16_SCALED", "1") != "0"     # measurement knob: the constants behind the pairs

    # ---- deferred status word ---------------------------------------------------------------
    def flags(self, device):
        key = torch.device(device).index
        if key is None:
            key = torch.cuda.current_device()
        word = self._flags.get(key)
        if word is None:
            with self._lock:
                word = self._flags.get(key)
                if word is None:
                    word = torch.zeros(1, dtype=torch.int32, device=torch.device("cuda", key))
                    self._flags[key] = word
        return word

    def read_flags(self, device):
        """Synchronising read-and-clear of the device status word."""
        word = self.flags(device)
        value = int(word.item())
        if value:
            word.zero_()
        return value

    def discard_flags(self):
        """Clears every device's status word without synchronising (an `infer` was abandoned half way:
        what its kernels flagged must not surface in the next call).  Skipped during a capture."""
        for index, word in list(self._flags.items()):
            with torch.cuda.device(index):
                if not torch.cuda.is_current_stream_capturing():
                    word.zero_()

    def _flag_unless_all(self, valid, bit):
        """ORs `bit` into the status word unless every element of the boolean tensor `valid` is True — device-side, no
        synchronisation, three small launches (all, select, or)."""
        device = valid.device
        constants = self._flag_constants.get((device, bit))
        if constants is None:
            constants = self._flag_constants[(device, bit)] = (
                torch.zeros((), dtype=torch.int32, device=device), torch.full((), bit, dtype=torch.int32, device=device))
        self.flags(device).bitwise_or_(torch.where(valid.all(), constants[0], constants[1]))

    def defer_support_check(self, valid):
        """FLAG_VALUE_OUTSIDE_SUPPORT unless all of `valid` (a value against a distribution's support) holds."""
        self._flag_unless_all(valid, _lib.FLAG_VALUE_OUTSIDE_SUPPORT)

    def defer_parameter_check(self, valid):
        """FLAG_INVALID_PARAMETER unless all of `valid` (a distribution parameter against its constraint) holds."""
        self._flag_unless_all(valid, _lib.FLAG_INVALID_PARAMETER)

    @staticmethod
    def _stream(t):
        # the raw handle of torch's current stream on t's device (torch.cuda.current_stream builds a Stream
        # object around the same call: 3 us of host time per launch)
        if _raw_stream is not None:
            return _raw_stream(t.device.index if t.device.index is not None else torch.cuda.current_device())
        return torch.cuda.current_stream(t.device).cuda_stream

    # ---- the one launch path and the operand checks the wrappers share -------------------------
    def _launch(self, device, entry, args, nbytes=None, keep=(), name=None, decline=False):
        """Enqueues `entry(*args)` (a C-ABI entry point; the stream is the LAST of `args`) with `device` current and
        raises on a failing status.  `decline`: the library's "unsupported shape" (nothing was launched) returns False
        instead, for the caller's other route.  With a KernelTimer installed the launch is recorded under `name` (default:
        the entry point's name without "aesmc_"), `nbytes()` its algorithmic traffic, `keep` everything whose address
        is in `args` (the timer replays them after the caller has returned); `nbytes` None: never timed."""
        with _on_device(device):
            status = entry(*args)
        if status != _lib.OK:
            if decline and status == _lib.ERR_UNSUPPORTED:
                return False
            _lib.check(status, entry.__name__)
        if self.timer is not None and nbytes is not None:
            self.timer.note(name or entry.__name__[6:], (entry, args), nbytes(), keep)
        return True

    @staticmethod
    def _expect(t, shape, like, what):
        """ValueError unless `t` has `shape` and `like`'s dtype and device."""
        if t.shape != shape or t.dtype != like.dtype or t.device != like.device:
            raise ValueError("aesmc_amd: {} must be {} {} on {}, got {} {} on {}".format(
                what, tuple(shape), like.dtype, like.device, tuple(t.shape), t.dtype, t.device))

    @staticmethod
    def _rows_operand(t, what):
        """The dtype tag of a [batch_size, num_particles] float tensor on the HIP device."""
        _require_hip(t, what)
        tag = _tag(t, what)
        if t.dim() != 2:
            raise ValueError("aesmc_amd: {} must be [batch_size, num_particles], got {}".format(what, tuple(t.shape)))
        return tag

    def _resampling_operands(self, log_w, u):
        """(tag, B, K, stratified) of K2's operands: log_w [B,K] float32/64, u float64 on its device.  The SHAPE of the
        uniforms names the scheme: B values (one per batch row) — systematic; [B,K] (one per particle) — stratified."""
        _require_hip(log_w, "log_weight")
        _require_hip(u, "uniforms")
        tag = self._rows_operand(log_w, "log_weight")
        B, K = log_w.shape
        stratified = u.dim() == 2 and tuple(u.shape) == (B, K)      # (K == 1: the two schemes are the same function)
        if u.dtype != torch.float64 or u.device != log_w.device or not (stratified or u.numel() == B):
            raise ValueError("aesmc_amd: uniforms must be {} float64 values (systematic) or [{}, {}] float64 (stratified) "
                             "on {}".format(B, B, K, log_w.device))
        return tag, B, K, stratified

    def _stratified(self, tag, log_w, u, B, K, want_lse, want_child_end, decline):
        """The one launch of the stratified scheme (aesmc_resample_step_stratified): (idx, lse, child_end), or None where
        the library declines (`decline`: by-products beyond the in-workgroup limit)."""
        idx = torch.empty((B, K), dtype=torch.int64, device=log_w.device)
        lse = torch.empty((B,), dtype=log_w.dtype, device=log_w.device) if want_lse else None
        child_end = torch.empty((B, K), dtype=torch.int32, device=log_w.device) if want_child_end else None
        if idx.numel() == 0:
            return idx, lse, child_end
        ws_bytes = int(self._lib.aesmc_workspace_bytes(B, K))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=log_w.device) if ws_bytes else None
        # the systematic step's 12 B per particle plus one float64 uniform each
        nbytes = lambda: B * K * (log_w.element_size() + 16) + (4 * B * K if child_end is not None else 0) + \
            (B * log_w.element_size() if lse is not None else 0)
        if not self._launch(log_w.device, self._lib.aesmc_resample_step_stratified,
                            (tag, _ptr(log_w), _ptr(u), _ptr(idx), _ptr(lse), _ptr(child_end),
                             _ptr(self.flags(log_w.device)), B, K, _ptr(ws), ws_bytes, self._stream(log_w)),
                            nbytes, (log_w, u, idx, lse, child_end, ws), name="resample_step_stratified", decline=decline):
            return None
        idx._aesmc_sorted = True  # one position per stratum: monotone in k, like the systematic scheme
        if child_end is not None:
            idx._aesmc_child_end = child_end
        return idx, lse, child_end

    # ---- K1 ------------------------------------------------------------------------------------
    def logweight_lse(self, a, b=None, c=None, want_lw=True, want_lse=True):
        """lw = a + b - c over [B,K]; lse[b] = logsumexp_k lw.  Returns (lw or None, lse or None)."""
        tag = self._rows_operand(a, "log-prob terms")
        for t in (b, c):
            if t is not None:
                _require_hip(t, "log-prob term")
                self._expect(t, a.shape, a, "log-prob term")
        a, b, c = [None if t is None else t.contiguous() for t in (a, b, c)]
        B, K = a.shape
        if b is None and c is None and not want_lse:
            return (a if want_lw else None), None
        need_lw = want_lw and not (b is None and c is None)
        lw = torch.empty_like(a) if need_lw else None
        lse = torch.empty(B, dtype=a.dtype, device=a.device) if want_lse else None
        esz = a.element_size()
        self._launch(a.device, self._lib.aesmc_logweight_lse,
                     (tag, _ptr(a), _ptr(b), _ptr(c), _ptr(lw), _ptr(lse), B, K, self._stream(a)),
                     lambda: B * K * esz * (1 + (b is not None) + (c is not None) + (lw is not None)) + B * esz,
                     (a, b, c, lw, lse))
        if want_lw and not need_lw:
            lw = a
        return lw, lse

    def logweight_accumulate(self, a, b, c, acc, want_lw=True, want_lse=False):
        """K1 with the running sum over time of importance sampling: lw = a + b - c (b, c optional),
        total = acc + lw, lse[b] = logsumexp_k total.  Returns (lw or None, total, lse or None)."""
        tag = self._rows_operand(a, "log-prob terms")
        for t in (b, c, acc):
            if t is not None:
                _require_hip(t, "log-prob term")
                self._expect(t, a.shape, a, "log-prob term")
        if acc is None:
            raise ValueError("aesmc_amd: logweight_accumulate needs the running sum")
        a, b, c, acc = [None if t is None else t.contiguous() for t in (a, b, c, acc)]
        B, K = a.shape
        need_lw = want_lw and not (b is None and c is None)
        lw = torch.empty_like(a) if need_lw else None
        total = torch.empty_like(a)
        lse = torch.empty(B, dtype=a.dtype, device=a.device) if want_lse else None
        if a.numel() == 0:
            return (lw if need_lw else (a if want_lw else None)), total, lse
        esz = a.element_size()
        self._launch(a.device, self._lib.aesmc_logweight_accumulate,
                     (tag, _ptr(a), _ptr(b), _ptr(c), _ptr(acc), _ptr(lw), _ptr(total), _ptr(lse), B, K, self._stream(a)),
                     lambda: B * K * esz * (3 + (b is not None) + (c is not None) + (lw is not None)) +
                     (B * esz if want_lse else 0), (a, b, c, acc, lw, total, lse))
        if want_lw and not need_lw:
            lw = a
        return lw, total, lse

    def logweight_lse_backward(self, lw, lse, grad_lw, grad_lse, want_neg=True):
        tag = self._rows_operand(lw, "lw")
        B, K = lw.shape
        lw = lw.contiguous()
        lse = lse.contiguous()
        self._expect(lse, (B,), lw, "lse")
        if grad_lw is not None:
            self._expect(grad_lw, lw.shape, lw, "grad_lw")
            grad_lw = grad_lw.contiguous()
        if grad_lse is not None:
            self._expect(grad_lse, (B,), lw, "grad_lse")
            grad_lse = grad_lse.contiguous()
        g = torch.empty_like(lw)
        ng = torch.empty_like(lw) if want_neg else None
        self._launch(lw.device, self._lib.aesmc_logweight_lse_backward,
                     (tag, _ptr(lw), _ptr(lse), _ptr(grad_lw), _ptr(grad_lse), _ptr(g), _ptr(ng), B, K, self._stream(lw)),
                     lambda: B * K * lw.element_size() * (2 + (grad_lw is not None) + (ng is not None)),
                     (lw, lse, grad_lw, grad_lse, g, ng))
        return g, ng

    # ---- K2 ------------------------------------------------------------------------------------
    def ancestor_index(self, log_w, u):
        """log_w [B,K] float32/64, u float64 (both on the HIP device) -> int64 [B,K].  u [B]: systematic resampling
        (one uniform per batch row); u [B,K]: stratified (one per particle)."""
        tag, B, K, stratified = self._resampling_operands(log_w, u)
        log_w = log_w.contiguous()
        u = u.contiguous()
        if stratified:
            return self._stratified(tag, log_w, u, B, K, False, False, decline=False)[0]
        idx = torch.empty((B, K), dtype=torch.int64, device=log_w.device)
        ws_bytes = int(self._lib.aesmc_workspace_bytes(B, K))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=log_w.device) if ws_bytes else None
        self._launch(log_w.device, self._lib.aesmc_ancestor_index,
                     (tag, _ptr(log_w), _ptr(u), _ptr(idx), _ptr(self.flags(log_w.device)), B, K, _ptr(ws), ws_bytes,
                      self._stream(log_w)),
                     lambda: B * K * (log_w.element_size() + 8) + 8 * B, (log_w, u, idx, ws))
        idx._aesmc_sorted = True  # systematic resampling is monotone in k: lets K3's backward skip atomics
        return idx

    # A workgroup owns a whole batch row: copying the payload inside the step pays while one row's
    # payload is small next to the chip (measured: 160 KB rows at B >= 128 gain, 8 MB rows lose 2x).
    STEP_PAYLOAD_MAX_ROW_BYTES = 1 << 20

    def step_covers(self, log_w, payload=None):
        """Host-only: can `resample_step` take this log-weight tensor (and payload)?"""
        if not (log_w.is_cuda and log_w.dim() == 2 and log_w.dtype in _DTYPE_TAG):
            return False
        K = log_w.size(1)
        if K > self.lds_max_particles or log_w.numel() == 0:
            return False
        if payload is None:
            return True
        if not (torch.is_tensor(payload) and payload.is_cuda and payload.device == log_w.device and
                payload.size()[:2] == log_w.size() and payload.numel() > 0 and _inner_dense(payload)):
            return False
        esz = payload.element_size()
        row_bytes = esz * (payload[0, 0].numel())
        if row_bytes % 4 or (K * row_bytes) % 16 or K * row_bytes > self.STEP_PAYLOAD_MAX_ROW_BYTES:
            return False
        return all((x * esz) % 4 == 0 for x in (payload.stride(0), payload.stride(1))) and \
            payload.data_ptr() % 4 == 0

    def step_packs(self, B, K, log_w):
        """Host-only: does aesmc_resample_step_packed take rows of K particles — whole wavefronts of the lean kernel's
        particles per lane, and more than 512 particles: exactly where `resample_step` without a payload runs that kernel
        itself (the header's rule), so the packed and the unpacked step are one kernel body with two output forms."""
        if not 512 < K <= self.lds_max_particles or B < 1 or log_w.data_ptr() % 16:
            return False
        per_lane = 4 if (K <= 4096 and K % 256 == 0) else (4 if K <= 2048 else (8 if K <= 8192 else (16 if K <= 16384 else 32)))
        return K % (64 * per_lane) == 0 and K // per_lane <= 1024

    def unpack_ancestors(self, words, want_child_end=True):
        """(idx int64 [B,K], child_end int32 [B,K] or None) of the packed words: one launch (aesmc_unpack_ancestors)."""
        B, K = words.shape
        idx = torch.empty((B, K), dtype=torch.int64, device=words.device)
        ends = torch.empty((B, K), dtype=torch.int32, device=words.device) if want_child_end else None
        if idx.numel():
            self._launch(words.device, self._lib.aesmc_unpack_ancestors,
                         (_ptr(words), _ptr(idx), _ptr(ends), B, K, self._stream(words)),
                         lambda: B * K * (12 + (4 if ends is not None else 0)), (words, idx, ends), name="unpack_ancestors")
        return idx, ends

    def resample_step(self, log_w, u, payload=None, want_lse=False, want_child_end=False, packed=False):
        """The fused step: (idx, lse, resampled payload) from one launch — idx as `ancestor_index`,
        lse = logsumexp over particles [B] when `want_lse`, payload[b, idx[b,k]] as `gather` when a
        payload tensor [B,K,...] is given (else None).  Returns None when the launch does not cover
        the operands (more particles than one workgroup holds, payload rows not 4-byte multiples):
        the caller then runs `ancestor_index` / `gather` / `logweight_lse` separately.
        u [B,K] (stratified resampling): the stratified launch, which has no payload tail — `moved` is None whatever
        payload was offered and the caller gathers with the indices.
        `packed` (no payload, systematic): where `step_packs` holds, idx comes back as a `PackedAncestors` — the indices
        and, with `want_child_end`, the ranges in one word per particle."""
        tag, B, K, stratified = self._resampling_operands(log_w, u)
        if K > self.lds_max_particles:
            return None
        log_w = log_w.contiguous()
        u = u.contiguous()
        if packed and payload is None and not stratified and self.step_packs(B, K, log_w):
            words = torch.empty((B, K), dtype=torch.int32, device=log_w.device)
            lse = torch.empty((B,), dtype=log_w.dtype, device=log_w.device) if want_lse else None
            if self._launch(log_w.device, self._lib.aesmc_resample_step_packed,
                            (tag, _ptr(log_w), _ptr(u), _ptr(words), _ptr(lse), 1 if want_child_end else 0,
                             _ptr(self.flags(log_w.device)), B, K, self._stream(log_w)),
                            lambda: B * K * (log_w.element_size() + 8) + 8 * B + (4 * B * K if want_child_end else 0),
                            (log_w, u, words, lse, None, None, None), name="resample_step", decline=True):
                return PackedAncestors(words, want_child_end), lse, None
        if stratified:
            if log_w.numel() == 0:
                return None
            out = self._stratified(tag, log_w, u, B, K, want_lse, want_child_end, decline=True)
            return None if out is None else (out[0], out[1], None)
        row_bytes = sb = sk = 0
        dst = None
        if payload is not None:
            _require_hip(payload, "value")
            assert payload.size()[:2] == log_w.size()
            if payload.device != log_w.device:
                raise RuntimeError("aesmc_amd: value on {} but log_weight on {}".format(payload.device,
                                                                                   log_w.device))
            if not _inner_dense(payload):
                payload = payload.contiguous()
            esz = payload.element_size()
            row_bytes = esz
            for size in payload.shape[2:]:
                row_bytes *= size
            sb, sk = payload.stride(0) * esz, payload.stride(1) * esz
            dst = torch.empty(payload.shape, dtype=payload.dtype, device=payload.device)
            if dst.numel() == 0:
                payload = dst = None
        idx = torch.empty((B, K), dtype=torch.int64, device=log_w.device)
        lse = torch.empty((B,), dtype=log_w.dtype, device=log_w.device) if want_lse else None
        if idx.numel() == 0:
            return None
        child_end = None
        flags = self.flags(log_w.device)
        if want_child_end and dst is None:
            # the children ranges ride along (aesmc_resample_step_ranges): where each particle's children end, for
            # the propagation's backward, which sums a particle's children itself (`idx._aesmc_child_end`)
            child_end = torch.empty((B, K), dtype=torch.int32, device=log_w.device)
            entry = self._lib.aesmc_resample_step_ranges
            args = (tag, _ptr(log_w), _ptr(u), _ptr(idx), _ptr(lse), _ptr(child_end), _ptr(flags), B, K,
                    self._stream(log_w))
        else:
            entry = self._lib.aesmc_resample_step
            args = (tag, _ptr(log_w), _ptr(u), _ptr(idx), _ptr(lse), _ptr(payload if dst is not None else None),
                    _ptr(dst), _ptr(flags), B, K, row_bytes, sb, sk, self._stream(log_w))
        # K2's 12 B + K3's (8 + 2 row_bytes) per particle when the payload rides along
        nbytes = lambda: B * K * (log_w.element_size() + 8) + 8 * B + \
            (B * K * (8 + 2 * row_bytes) if dst is not None else 0) + (4 * B * K if child_end is not None else 0)
        if not self._launch(log_w.device, entry, args, nbytes, (log_w, u, idx, lse, payload, dst, child_end),
                            name="resample_step", decline=True):
            return None
        idx._aesmc_sorted = True
        if child_end is not None:
            idx._aesmc_child_end = child_end
        return idx, lse, dst

    # ---- K3 ------------------------------------------------------------------------------------
    @staticmethod
    def _check_index(value, idx):
        _require_hip(idx, "ancestral_index")
        if idx.dtype != torch.int64:
            raise TypeError("aesmc_amd: ancestral_index must be int64 (torch.LongTensor), got {}"
                            .format(idx.dtype))
        if idx.device != value.device:
            raise RuntimeError("aesmc_amd: ancestral_index on {} but value on {}".format(
                idx.device, value.device))

    def _ancestors(self, value, ancestors, B, K, what):
        """The indices a fused launch fetches `value`'s rows through (int64 [B,K] on value's device), dense; None stays
        None."""
        if ancestors is None:
            return None
        ancestors = as_index(ancestors)
        self._check_index(value, ancestors)
        if ancestors.shape != (B, K):
            raise ValueError("aesmc_amd: {} ancestors must be [{}, {}]".format(what, B, K))
        return ancestors.contiguous()

    def gather(self, src, idx):
        """dst[b,k,...] = src[b, idx[b,k], ...]; src [B,K,...] any dtype, idx int64 [B,K]."""
        _require_hip(src, "value")
        idx = as_index(idx)
        self._check_index(src, idx)
        assert idx.size() == src.size()[:2]
        B, K = idx.shape
        if not _inner_dense(src):
            src = src.contiguous()  # trailing dims must be dense; the leading two may be strided
        row_elems = 1
        for s in src.shape[2:]:
            row_elems *= s
        esz = src.element_size()
        dst = torch.empty(src.shape, dtype=src.dtype, device=src.device)
        if dst.numel() == 0:
            return dst
        idx = idx.contiguous()
        self._launch(src.device, self._lib.aesmc_resample_gather,
                     (_ptr(src), _ptr(idx), _ptr(dst), _ptr(self.flags(src.device)), B, K, row_elems * esz,
                      src.stride(0) * esz, src.stride(1) * esz, self._stream(src)),
                     lambda: B * K * (8 + 2 * row_elems * esz), (src, idx, dst))
        return dst

    def gather_backward(self, grad_out, idx, sorted_index=False):
        """grad_src[b,j,...] = sum over {k: idx[b,k]==j} of grad_out[b,k,...].  `sorted_index`
        promises idx non-decreasing along k (outputs of `ancestor_index`): segmented sum, no atomics."""
        _require_hip(grad_out, "grad")
        idx = as_index(idx)
        self._check_index(grad_out, idx)
        tag = _tag(grad_out, "gradient of a resampled value")
        B, K = idx.shape
        grad_out = grad_out.contiguous()
        idx = idx.contiguous()
        row_elems = 1
        for s in grad_out.shape[2:]:
            row_elems *= s
        # The sorted-index kernel writes every row of the result exactly once — if the promise holds.  Indices K2 wrote
        # itself keep it by construction; a tag that was only INHERITED (a lineage composed from tagged indices, or one a
        # caller set) starts from zeros, so that a false promise leaves zero rows behind its flag, not stale memory.
        grad_src = torch.zeros_like(grad_out) if sorted_index == "inherited" else torch.empty_like(grad_out)
        if grad_src.numel() == 0:
            return grad_src
        self._launch(grad_out.device, self._lib.aesmc_resample_gather_backward,
                     (tag, _ptr(grad_out), _ptr(idx), _ptr(grad_src), _ptr(self.flags(grad_out.device)), B, K, row_elems,
                      1 if sorted_index else 0, self._stream(grad_out)),
                     lambda: B * K * (8 + 2 * row_elems * grad_out.element_size()), (grad_out, idx, grad_src))
        return grad_src


    def gather_backward_ranges(self, child_grad, child_end):
        """grad_src[b,k] = sum of child_grad[b, child_end[b,k-1] : child_end[b,k]] — torch.gather's backward stated with
        the children ranges instead of the indices (only for shapes the fused backward declines)."""
        if type(child_end) is PackedAncestors:
            child_end = child_end.child_end()
        B, K = child_end.shape
        ends = child_end.to(torch.int64)
        position = torch.arange(K, device=child_end.device).unsqueeze(0).expand(B, K).contiguous()
        # the ancestor of position k is the number of particles whose children end at or before k
        index = torch.searchsorted(ends, position, right=True).clamp_(max=K - 1)
        return self.gather_backward(child_grad, index, sorted_index=True)

    # ---- K4 ------------------------------------------------------------------------------------
    @staticmethod
    def _view3(t):
        """Describes a [B,K,*] tensor as (tensor, (sb, sk, sd), D) with the trailing dims collapsed
        into one of extent D and element stride sd (0 = broadcast).  Copies only when the trailing
        dims cannot be described by a single stride."""
        rank = t.dim()
        if rank == 3:                     # the usual case: nothing to collapse
            return t, t.stride(), t.size(2)
        if rank == 2:
            return t, t.stride() + (0,), 1
        D = 1
        for size in t.shape[2:]:
            D *= size
        dims = [(size, stride) for size, stride in zip(t.shape[2:], t.stride()[2:]) if size != 1]
        for (_, outer), (size, inner) in zip(dims, dims[1:]):
            if outer != inner * size:
                t = t.contiguous()
                return t, (t.stride(0), t.stride(1), 1), D
        sd = dims[-1][1] if dims else 0
        return t, (t.stride(0), t.stride(1), sd), D

    @staticmethod
    def _unique_bytes(t):
        n = t.element_size()
        for size, stride in zip(t.shape, t.stride()):
            if stride != 0:
                n *= size
        return n

    def _normal_operands(self, value, loc, scale):
        _require_hip(value, "value")
        tag = _tag(value, "value")
        if value.dim() < 2:
            raise ValueError("aesmc_amd: value must be [batch_size, num_particles, ...]")
        for name, t in (("loc", loc), ("scale", scale)):
            _require_hip(t, name)
            self._expect(t, value.shape, value, name)
        (value, sv, D), (loc, sm, _), (scale, ss, _) = [self._view3(t) for t in (value, loc, scale)]
        return tag, value, loc, scale, sv, sm, ss, D

    def normal_logprob_sum(self, value, loc, scale):
        """sum over trailing dims of Normal(loc, scale).log_prob(value) -> [B,K]; loc and scale are
        views already expanded to value's shape (stride 0 where broadcast)."""
        tag, value, loc, scale, sv, sm, ss, D = self._normal_operands(value, loc, scale)
        B, K = value.shape[:2]
        out = torch.empty((B, K), dtype=value.dtype, device=value.device)
        if out.numel() == 0:
            return out
        self._launch(value.device, self._lib.aesmc_normal_logprob_sum,
                     (tag, _ptr(value), _ptr(loc), _ptr(scale), _ptr(out), B, K, D) + sv + sm + ss + (self._stream(value),),
                     lambda: sum(self._unique_bytes(t) for t in (value, loc, scale)) + out.numel() * out.element_size(),
                     (value, loc, scale, out))
        return out

    def normal_logprob_sum_backward(self, value, loc, scale, grad_out, need_value, need_loc, need_scale):
        """Dense [B,K,*] gradients w.r.t. value / loc / scale (None where not needed)."""
        shape = value.shape
        tag, value, loc, scale, sv, sm, ss, D = self._normal_operands(value, loc, scale)
        B, K = shape[:2]
        self._expect(grad_out, (B, K), value, "grad_out")
        grad_out = grad_out.contiguous()
        outs = [torch.empty(shape, dtype=value.dtype, device=value.device) if need else None
                for need in (need_value, need_loc, need_scale)]
        if value.numel() == 0 or not any(o is not None for o in outs):
            return tuple(None if o is None else o.zero_() for o in outs)
        self._launch(value.device, self._lib.aesmc_normal_logprob_sum_backward,
                     (tag, _ptr(value), _ptr(loc), _ptr(scale), _ptr(grad_out), _ptr(outs[0]), _ptr(outs[1]),
                      _ptr(outs[2]), B, K, D) + sv + sm + ss + (self._stream(value),),
                     lambda: sum(self._unique_bytes(t) for t in (value, loc, scale, grad_out)) +
                     sum(o.numel() * o.element_size() for o in outs if o is not None),
                     (value, loc, scale, grad_out) + tuple(outs))
        return tuple(outs)


    # ---- K5 ------------------------------------------------------------------------------------
    @staticmethod
    def normal_logweight_covers(x, scale_p, y, scale_g, scale_q):
        """Host-only pre-test of K5's preconditions: HIP float tensors of equal leading shape, at
        least one value per particle.  The launch itself may still decline (wide rows that are not
        whole 16-byte vectors, wide rows with tensor scales): `normal_logweight` then returns None."""
        if not (x.is_cuda and y.is_cuda and x.dtype in _DTYPE_TAG and y.dtype == x.dtype):
            return False
        if x.dim() < 2 or y.dim() < 2 or x.shape[:2] != y.shape[:2] or x.device != y.device:
            return False
        return x.numel() != 0 and y.numel() != 0

    def normal_logweight(self, x, loc_p, scale_p, y, loc_g, scale_g, loc_q, scale_q):
        """lw = logN(x; loc_p, scale_p) + logN(y; loc_g, scale_g) - logN(x; loc_q, scale_q), each
        summed over trailing dims -> [B,K]; loc / scale are views expanded to x's (resp. y's) shape.
        Returns None when the kernel does not cover the operands (wide rows that are not whole
        aligned 16-byte vectors, or wide rows with tensor scales):
        the caller then takes the K4 + K1 route, which gives bit-identical numbers."""
        tag, x, loc_p, scale_p, sx, sp, ssp, Dx = self._normal_operands(x, loc_p, scale_p)
        _, y, loc_g, scale_g, sy, sg, ssg, Dy = self._normal_operands(y, loc_g, scale_g)
        _, x2, loc_q, scale_q, sx2, sq, ssq, _ = self._normal_operands(x, loc_q, scale_q)
        if y.dtype != x.dtype or y.device != x.device or y.shape[:2] != x.shape[:2]:
            return None
        if Dx < 1 or Dy < 1:
            return None
        if x2 is not x and x2.data_ptr() != x.data_ptr():    # _view3 had to copy x: keep one copy
            x2, sx2 = x, sx
        B, K = x.shape[:2]
        out = torch.empty((B, K), dtype=x.dtype, device=x.device)
        if out.numel() == 0:
            return out
        views = (_lib.View3 * 8)(*[_lib.View3(_ptr(t), *st) for t, st in (
            (x, sx), (loc_p, sp), (scale_p, ssp), (y, sy), (loc_g, sg), (scale_g, ssg), (loc_q, sq),
            (scale_q, ssq))])
        if not self._launch(x.device, self._lib.aesmc_normal_logweight,
                            (tag, views, _ptr(out), B, K, Dx, Dy, self._stream(x)),
                            lambda: sum(self._unique_bytes(t) for t in (x, loc_p, y, loc_g, loc_q)) +
                            out.numel() * out.element_size(),
                            (x, loc_p, scale_p, y, loc_g, scale_g, loc_q, scale_q, out, views), decline=True):
            return None
        return out

    def normal_logweight_backward(self, x, loc_p, scale_p, y, loc_g, scale_g, loc_q, scale_q, grad_lw, need,
                                  lw=None, lse=None, grad_lse=None):
        """Gradients of `normal_logweight` in one launch: dense [B,K,*] tensors in the order
        (x, loc_p, scale_p, y, loc_g, scale_g, loc_q, scale_q), None where `need[i]` is false.
        With `lw`, `lse`, `grad_lse` the incoming gradient is K1's backward formed in place,
        grad_lse[b] * exp(lw - lse[b]) (+ grad_lw if given): the per-step softmax term never goes
        through HBM as a [B,K] tensor."""
        tag, x, loc_p, scale_p, sx, sp, ssp, Dx = self._normal_operands(x, loc_p, scale_p)
        _, y, loc_g, scale_g, sy, sg, ssg, Dy = self._normal_operands(y, loc_g, scale_g)
        _, _, loc_q, scale_q, _, sq, ssq, _ = self._normal_operands(x, loc_q, scale_q)
        if Dx < 1 or Dy < 1:
            return None
        B, K = x.shape[:2]
        fused_lse = grad_lse is not None
        if fused_lse:
            lw, lse, grad_lse = lw.contiguous(), lse.contiguous(), grad_lse.contiguous()
            self._expect(lw, (B, K), x, "lw")
            self._expect(lse, (B,), x, "lse")
            self._expect(grad_lse, (B,), x, "grad_lse")
        if grad_lw is not None:
            grad_lw = grad_lw.contiguous()
        elif not fused_lse:
            raise ValueError("aesmc_amd: normal_logweight_backward needs grad_lw or (lw, lse, grad_lse)")
        make = lambda like, wanted: torch.empty(like.shape, dtype=like.dtype, device=like.device) if wanted else None
        outs = [make(x, need[0]), make(x, need[1]), make(x, need[2]), make(y, need[3]), make(y, need[4]),
                make(y, need[5]), make(x, need[6]), make(x, need[7])]
        if x.numel() == 0:
            return outs
        gx, gp, gsp, gy, gg, gsg, gq, gsq = outs
        views = (_lib.View3 * 8)(*[_lib.View3(_ptr(t), *st) for t, st in (
            (x, sx), (loc_p, sp), (scale_p, ssp), (y, sy), (loc_g, sg), (scale_g, ssg), (loc_q, sq),
            (scale_q, ssq))])
        tail = (_ptr(gx), _ptr(gp), _ptr(gy), _ptr(gg), _ptr(gq), _ptr(gsp), _ptr(gsg), _ptr(gsq), B, K, Dx, Dy,
                self._stream(x))
        if fused_lse:
            entry = self._lib.aesmc_normal_logweight_lse_backward
            args = (tag, views, _ptr(lw), _ptr(lse), _ptr(grad_lse), _ptr(grad_lw)) + tail
        else:
            entry = self._lib.aesmc_normal_logweight_backward
            args = (tag, views, _ptr(grad_lw)) + tail
        reads = (x, loc_p, scale_p, y, loc_g, scale_g, loc_q, scale_q, grad_lw, lw)
        if not self._launch(x.device, entry, args,
                            lambda: sum(self._unique_bytes(t) for t in reads if t is not None) +
                            sum(t.numel() * t.element_size() for t in outs if t is not None),
                            reads + (lse, grad_lse, views) + tuple(outs), decline=True):
            return None
        return outs

    def normal_rsample(self, eps, loc, scale):
        """loc + eps * scale (product rounded first, as eager PyTorch) -> DENSE tensor of eps's
        shape [B,K,*]; loc and scale are views already expanded to that shape.  eps may be the
        transposed view of a [K,B,*] draw: the result is written in [B,K,*] order directly."""
        tag = _DTYPE_TAG[eps.dtype]
        (eps, se, D), (loc, sm, _), (scale, ss, _) = [self._view3(t) for t in (eps, loc, scale)]
        B, K = eps.shape[:2]
        out = torch.empty(eps.shape, dtype=eps.dtype, device=eps.device)
        if out.numel() == 0:
            return out
        def launch(eps, se, decline):
            views = [_lib.View3(_ptr(t), *st) for t, st in ((eps, se), (loc, sm), (scale, ss))]
            return self._launch(eps.device, self._lib.aesmc_normal_rsample,
                                (tag, ctypes.byref(views[0]), ctypes.byref(views[1]), ctypes.byref(views[2]), _ptr(out),
                                 B, K, D, self._stream(eps)),
                                lambda: sum(self._unique_bytes(t) for t in (eps, loc, scale)) + out.numel() * out.element_size(),
                                (eps, loc, scale, out, views), decline=decline)
        if not launch(eps, se, decline=True):
            eps = eps.contiguous()   # a noise layout the kernel does not know: materialise it
            launch(eps, (eps.stride(0), eps.stride(1), 1), decline=False)
        return out

    # Below this many elements the noise launch + K6 pair is as fast (both are launch-latency bound) and the drawn
    # kernel's 4-byte accesses buy nothing.
    RSAMPLE_DRAWN_MIN_ELEMENTS = int(settings.knob("AESMC_RSAMPLE_DRAWN_MIN", str(1 << 18)))

    def normal_rsample_drawn(self, noise, loc, scale, shape):
        """K6 with the noise formed in the launch: loc + n * scale -> dense float32 [B,K,*] of `shape`, n being the
        tensor `torch.empty(shape).normal_()` would have held for the reservation `noise` (an `_philox.NoiseStream`);
        loc and scale are views already expanded to `shape`.  None where the launch does not apply (the caller draws
        the noise with `philox_normal` and takes `normal_rsample`)."""
        if loc.dtype != torch.float32 or len(shape) < 2:
            return None
        numel = 1
        for extent in shape:
            numel *= int(extent)
        if numel < self.RSAMPLE_DRAWN_MIN_ELEMENTS or numel >= (1 << 32) or numel != noise.numel:
            return None
        (loc, sm, D), (scale, ss, _) = [self._view3(t) for t in (loc, scale)]
        B, K = int(shape[0]), int(shape[1])
        out = torch.empty(tuple(shape), dtype=torch.float32, device=loc.device)
        views = [_lib.View3(_ptr(t), *st) for t, st in ((loc, sm), (scale, ss))]
        if not self._launch(loc.device, self._lib.aesmc_normal_rsample_drawn,
                            (_DTYPE_TAG[torch.float32], ctypes.byref(views[0]), ctypes.byref(views[1]), _ptr(out), B, K, D,
                             noise.seed, noise.offset, noise.threads, 0, _ptr(noise.state), self._stream(loc)),
                            lambda: self._unique_bytes(loc) + self._unique_bytes(scale) + 4 * numel,
                            (loc, scale, out, views), decline=True):
            return None
        return out

    # ---- K8 / K9 / K10: linear-Gaussian particle propagation -----------------------------------
    @property
    def affine_max_dim(self):
        if self._affine_max_dim is None:
            self._affine_max_dim = int(self._lib.aesmc_affine_max_dim())
        return self._affine_max_dim

    def affine_covers(self, source, weight, offset=None):
        """Host-only test of what K8 / K9 / K10 assume about one affine location
        `offset + source @ weight.T`: source [B,K,din] float32/64 on the HIP device, weight
        [dout,din] with din, dout <= aesmc_affine_max_dim(), offset None, [dout] or [B,dout]."""
        if not (torch.is_tensor(source) and torch.is_tensor(weight)):
            return False
        if not (source.is_cuda and source.dtype in _DTYPE_TAG and source.dim() == 3 and source.numel() > 0):
            return False
        if weight.dim() != 2 or weight.dtype != source.dtype or weight.device != source.device:
            return False
        dout, din = weight.shape
        if din != source.size(2) or not (1 <= din <= self.affine_max_dim and 1 <= dout <= self.affine_max_dim):
            return False
        if offset is not None:
            if not torch.is_tensor(offset) or offset.dtype != source.dtype or offset.device != source.device:
                return False
            if tuple(offset.shape) not in ((dout,), (source.size(0), dout)):
                return False
        return True

    @staticmethod
    def _dense16(t):
        """`t` laid out contiguously from a 16-byte aligned address (what the tile loads assume)."""
        t = t.contiguous()
        if t.data_ptr() % 16:
            t = t.clone(memory_format=torch.contiguous_format)
        return t

    def _affine_map(self, weight, offset, slot=None):
        """(aesmc_affine_map, tensors it borrows).  weight may be any 2-D view (a transpose costs
        nothing); offset is [dout] (shared by every batch row) or [B, dout].  `slot` (the hot per-timestep
        launchers pass the map's position in their argument list): the struct made for this weight tensor in
        this position is kept — a model hands the same parameters in at every timestep — and only its offset
        fields rewritten; the C entry points have read it by the time they return."""
        off_ptr, off_sb = 0, 0
        if offset is not None:
            if offset.stride(-1) != 1:
                offset = offset.contiguous()
            off_ptr = offset.data_ptr()
            off_sb = offset.stride(0) if offset.dim() == 2 else 0
        # (the timer keeps the structs of the launches it sampled; a view such as `A.t()` — a tensor with an autograd
        #  history — is never kept: a cache that outlives the step would keep that step's autograd graph alive, which
        #  a later hipGraph capture of a backward pass cannot tolerate)
        cached = slot is not None and self.timer is None and weight.grad_fn is None
        if cached:
            entry = self._map_cache.get((id(weight), slot))
            if entry is not None and entry[0] is weight and entry[1].weight == weight.data_ptr() and \
                    entry[2] == (weight.shape, weight.stride()):
                amap = entry[1]
                amap.offset, amap.offset_stride_b = off_ptr, off_sb
                return amap, (weight, offset)
        dout, din = weight.shape
        amap = _lib.AffineMap(weight.data_ptr(), weight.stride(0), weight.stride(1), off_ptr, off_sb, dout, din)
        if cached:
            if len(self._map_cache) > 64:
                self._map_cache.clear()
            self._map_cache[(id(weight), slot)] = (weight, amap, (weight.shape, weight.stride()))
        return amap, (weight, offset)

    @staticmethod
    def _map_args(maps, scales):
        """The three `_affine_map` results by reference, then (`scales` given) the three one-value scales: the argument
        block every three-map entry point takes."""
        refs = (ctypes.byref(maps[0][0]), ctypes.byref(maps[1][0]), ctypes.byref(maps[2][0]))
        return refs if scales is None else refs + (_ptr(scales[0]), _ptr(scales[1]), _ptr(scales[2]))

    @staticmethod
    def _unit_rows(y_rows):
        """The observation [B, dy] with unit element stride (its row stride is passed to the launch)."""
        return y_rows if y_rows.stride(1) == 1 else y_rows.contiguous()

    def particle_affine(self, x1, w1, offset=None, x2=None, w2=None, base=None, through_tanh=False):
        """K8: base + (offset + x1 @ w1.T + x2 @ w2.T) -> dense [B,K,dout]; x2 / w2, offset, base optional.
        Every element is one fma chain (w1's terms, then w2's) started from the offset.  `through_tanh`: the launch stores
        tanh of that (aesmc_particle_affine_tanh: the bits `torch.tanh` of the plain result holds)."""
        if not self.affine_covers(x1, w1, offset) or (x2 is not None and not self.affine_covers(x2, w2)):
            raise ValueError("aesmc_amd: particle_affine operands outside what kernel K8 covers")
        tag = _DTYPE_TAG[x1.dtype]
        B, K = x1.shape[:2]
        dout = w1.size(0)
        if x2 is not None and (x2.shape[:2] != x1.shape[:2] or w2.size(0) != dout or x2.dtype != x1.dtype):
            raise ValueError("aesmc_amd: particle_affine inputs disagree")
        x1 = self._dense16(x1)
        x2 = None if x2 is None else self._dense16(x2)
        if base is not None:
            self._expect(base, (B, K, dout), x1, "particle_affine base")
            base = self._dense16(base)
        out = torch.empty((B, K, dout), dtype=x1.dtype, device=x1.device)
        m1, keep1 = self._affine_map(w1, offset)
        m2, keep2 = self._affine_map(w2, None) if x2 is not None else (None, ())
        self._launch(x1.device, self._lib.aesmc_particle_affine_tanh if through_tanh else self._lib.aesmc_particle_affine,
                     (tag, _ptr(x1), ctypes.byref(m1), _ptr(x2), ctypes.byref(m2) if m2 is not None else None,
                      _ptr(base), _ptr(out), B, K, self._stream(x1)),
                     lambda: x1.element_size() * B * K * (x1.size(2) + (x2.size(2) if x2 is not None else 0) +
                                                          dout * (2 if base is not None else 1)),
                     (x1, x2, base, out, m1, m2, keep1, keep2), name="particle_affine")
        return out

    def affine_rsample(self, source, weight, offset, eps, scale, out=None):
        """K9: (offset + source @ weight.T) + eps * scale -> dense [B,K,dout]; `scale` holds one value.
        `out`: a dense, 16-byte aligned [B,K,dout] tensor to write instead of a new one."""
        if not self.affine_covers(source, weight, offset):
            raise ValueError("aesmc_amd: affine_rsample operands outside what kernel K9 covers")
        tag = _DTYPE_TAG[source.dtype]
        B, K = source.shape[:2]
        dout = weight.size(0)
        self._expect(eps, (B, K, dout), source, "affine_rsample noise")
        if scale.numel() != 1 or scale.dtype != source.dtype or scale.device != source.device:
            raise ValueError("aesmc_amd: affine_rsample takes one scale value on the device")
        source, eps = self._dense16(source), self._dense16(eps)
        if out is None:
            out = torch.empty((B, K, dout), dtype=source.dtype, device=source.device)
        else:
            self._check_out(out, (B, K, dout), source, "affine_rsample")
        amap, keep = self._affine_map(weight, offset)
        self._launch(source.device, self._lib.aesmc_affine_normal_rsample,
                     (tag, _ptr(source), ctypes.byref(amap), _ptr(eps), _ptr(scale), _ptr(out), B, K, self._stream(source)),
                     lambda: source.element_size() * B * K * (source.size(2) + 2 * dout),
                     (source, eps, scale, out, amap, keep))
        return out

    @staticmethod
    def _check_out(out, shape, like, what):
        if not (torch.is_tensor(out) and tuple(out.shape) == tuple(shape) and out.dtype == like.dtype and
                out.device == like.device and out.is_contiguous() and out.data_ptr() % 16 == 0):
            raise ValueError("aesmc_amd: {}: `out` must be a dense, 16-byte aligned {} {} tensor on {}".format(
                what, tuple(shape), like.dtype, like.device))

    def affine_propagate(self, x_prev, eps, y_rows, transition, emission, proposal, scales, out_x, checked=False,
                         ancestors=None):
        """K15: the proposal's draw and the step's log-weight in one launch.  Writes
        x = loc_q(x_prev) + eps * s_q into `out_x` (K9's bits) and returns K10's log-weight [B,K] of
        (x_prev, x, y_rows) (K10's bits).  `ancestors` (int64 [B,K]): `x_prev` is the UN-resampled latent and
        its rows are fetched through the indices inside the launch — x_prev[b, ancestors[b,k]] is never
        written; None comes back when the launch does not cover the shape (fewer than ~43 particles per
        batch row): the caller gathers, then calls again without `ancestors`."""
        # `checked`: the caller has just run affine_logweight_covers on these operands (x_t in eps's place)
        if not checked and not self.affine_logweight_covers(x_prev, eps, y_rows, transition, emission, proposal, scales):
            raise ValueError("aesmc_amd: affine_propagate operands outside what kernel K15 covers")
        self._expect(eps, x_prev.shape, x_prev, "affine_propagate noise")
        tag = _DTYPE_TAG[eps.dtype]
        B, K, dx = eps.shape
        self._check_out(out_x, (B, K, dx), eps, "affine_propagate")
        x_prev, eps = self._dense16(x_prev), self._dense16(eps)
        if out_x.data_ptr() == x_prev.data_ptr():
            raise ValueError("aesmc_amd: affine_propagate cannot write the draw over x_prev")
        ancestors = self._ancestors(x_prev, ancestors, B, K, "affine_propagate")
        y_rows = self._unit_rows(y_rows)
        out = torch.empty((B, K), dtype=eps.dtype, device=eps.device)
        maps = [self._affine_map(*term, slot=slot) for slot, term in enumerate((transition, emission, proposal))]
        tail = (_ptr(eps), _ptr(y_rows), y_rows.stride(0)) + self._map_args(maps, scales) + (_ptr(out_x), _ptr(out))
        if ancestors is not None:
            entry = self._lib.aesmc_affine_normal_propagate_resampled
            args = (tag, _ptr(x_prev), _ptr(ancestors)) + tail + (_ptr(self.flags(eps.device)), B, K, self._stream(eps))
        else:
            entry = self._lib.aesmc_affine_normal_propagate
            args = (tag, _ptr(x_prev)) + tail + (B, K, self._stream(eps))
        if not self._launch(eps.device, entry, args,
                            lambda: eps.element_size() * (B * K * (3 * dx + 1) + y_rows.numel()) +
                            (8 * B * K if ancestors is not None else 0),
                            (x_prev, ancestors, eps, y_rows, out, out_x, maps, scales), decline=ancestors is not None):
            return None
        return out

    # Particles below which the noise is materialised (aesmc_philox_normal_fill, the same values) and the step takes the
    # launches that read it instead of forming it in the propagation launch.  0 since round 5: with one work item per
    # workgroup (linear_gaussian_item.hip) the fused launch is ahead at every size measured, down to B=8 K=128 (5.6 us
    # against 3.0 + 7.3 for the fill followed by K15; B=256 K=1024: 14.6 against 6.2 + 13.8; profiles/r05_k16_small_shapes.txt).
    # Rounds 3 / 4 needed 1M / 0.5M particles for the persistent form to win.  Shapes the launch's item geometry does not
    # cover (fewer than 128 particles per row) are declined by the library and take the fill route as before.
    DRAWN_MIN_PARTICLES = int(settings.knob("AESMC_K16_MIN_PARTICLES", "0"))

    def philox_normal(self, stream_desc, shape, device):
        """The float32 tensor `torch.empty(shape).normal_()` would have held for the generator state
        `stream_desc` (an `_philox.NoiseStream`) — for a draw that was left to a kernel which then did not run."""
        out = torch.empty(shape, dtype=torch.float32, device=device)
        if out.numel() != stream_desc.numel:
            raise ValueError("aesmc_amd: noise of {} elements asked from a reservation of {}".format(
                out.numel(), stream_desc.numel))
        if out.numel() == 0:
            return out
        self._launch(out.device, self._lib.aesmc_philox_normal_fill,
                     (_ptr(out), out.numel(), stream_desc.seed, stream_desc.offset, stream_desc.threads, 0,
                      _ptr(stream_desc.state), self._stream(out)),
                     lambda: 4 * out.numel(), (out,))
        return out

    # ---- K13: two-layer tanh net over the particles ---------------------------------------------
    def particle_mlp_covers(self, x, weight1, offset1, weight2, bias2=None):
        """Host-only test of K13's preconditions: x [B,K,din] (din <= 16), weight1 [H,din] (H <= 64),
        offset1 [H] or [B,H], weight2 [dout,H] (dout <= 16), bias2 [dout] or None; at least ~43
        particles per batch row (the kernel stages the rows' offsets per 256-particle tile)."""
        if not (torch.is_tensor(x) and x.is_cuda and x.dtype in _DTYPE_TAG and x.dim() == 3 and x.numel() > 0):
            return False
        tensors = [weight1, offset1, weight2] + ([bias2] if bias2 is not None else [])
        if not all(torch.is_tensor(t) and t.dtype == x.dtype and t.device == x.device for t in tensors):
            return False
        if weight1.dim() != 2 or weight2.dim() != 2:
            return False
        H, din = weight1.shape
        dout = weight2.size(0)
        if din != x.size(2) or weight2.size(1) != H or not (1 <= din <= 16 and 1 <= dout <= 16 and 1 <= H <= 64):
            return False
        if tuple(offset1.shape) not in ((H,), (x.size(0), H)):
            return False
        if bias2 is not None and tuple(bias2.shape) != (dout,):
            return False
        return (256 - 1) // x.size(1) + 2 <= 8

    def particle_mlp(self, x, weight1, offset1, weight2, bias2=None):
        """K13: bias2 + tanh(offset1 + x @ weight1.T) @ weight2.T -> dense [B,K,dout]; None when the kernel
        declines the shape (the caller keeps the PyTorch expression)."""
        if not self.particle_mlp_covers(x, weight1, offset1, weight2, bias2):
            return None
        tag = _DTYPE_TAG[x.dtype]
        B, K = x.shape[:2]
        x = self._dense16(x)
        out = torch.empty((B, K, weight2.size(0)), dtype=x.dtype, device=x.device)
        m1, keep1 = self._affine_map(weight1, offset1)
        m2, keep2 = self._affine_map(weight2, bias2)
        if not self._launch(x.device, self._lib.aesmc_particle_mlp,
                            (tag, _ptr(x), ctypes.byref(m1), ctypes.byref(m2), _ptr(out), B, K, self._stream(x)),
                            lambda: x.element_size() * B * K * (x.size(2) + out.size(2)),
                            (x, out, m1, m2, keep1, keep2), decline=True):
            return None
        return out

    def particle_mlp_backward(self, grad_out, x, weight1, offset1, weight2, need_x=True):
        """K13b: for grad_out [B,K,dout] -> (grad_x [B,K,din] or None, grad_weight1 [H,din], grad_offset1 summed per batch
        row [B,H], grad_weight2 [dout,H]) with the hidden layer RECOMPUTED from x and offset1; None when the kernel
        declines the shape (K not a multiple of 256, din = 16: the caller differentiates the PyTorch expression)."""
        if not self.particle_mlp_covers(x, weight1, offset1, weight2) or grad_out.dtype != x.dtype or \
                grad_out.device != x.device or tuple(grad_out.shape) != (x.size(0), x.size(1), weight2.size(0)):
            return None
        B, K, din = x.shape
        H, dout = weight1.size(0), weight2.size(0)
        records = int(self._lib.aesmc_particle_mlp_backward_records(B, K))
        if records <= 0 or din > 15:
            return None
        tag = _DTYPE_TAG[x.dtype]
        x, grad_out = self._dense16(x), self._dense16(grad_out)
        chunks = (H + 15) // 16
        grad_x = torch.empty_like(x) if need_x else None
        rec_w1 = torch.empty((records, chunks, 16, 16), dtype=x.dtype, device=x.device)
        rec_w2 = torch.empty((records, chunks, 16, 16), dtype=x.dtype, device=x.device)
        rows = torch.empty((B, K // 64, 16 * chunks), dtype=x.dtype, device=x.device)
        m1, keep1 = self._affine_map(weight1, offset1)
        m2, keep2 = self._affine_map(weight2, None)
        if not self._launch(x.device, self._lib.aesmc_particle_mlp_backward,
                            (tag, _ptr(x), _ptr(grad_out), ctypes.byref(m1), ctypes.byref(m2), _ptr(grad_x), _ptr(rec_w1),
                             _ptr(rec_w2), _ptr(rows), B, K, self._stream(x)),
                            lambda: x.element_size() * B * K * (2 * din + dout),
                            (x, grad_out, grad_x, rec_w1, rec_w2, rows, m1, m2, keep1, keep2), decline=True):
            return None
        # the wavefronts' partials, added in record order; grad_W1's chunk c holds rows 16 c .. 16 c + 15 (hidden units) x
        # inputs, grad_W2's chunk c holds outputs x hidden units 16 c .. 16 c + 15
        grad_w1 = rec_w1.sum(0).reshape(16 * chunks, 16)[:H, :din]
        grad_w2 = rec_w2.sum(0).permute(1, 0, 2).reshape(16, 16 * chunks)[:dout, :H]
        grad_rows = rows.sum(1)[:, :H]
        return grad_x, grad_w1, grad_rows, grad_w2

    def _wide_limits(self):
        """(the extent with the noise in the launch and the backward pieces, smallest latent width, largest width) of the
        matrix-core step, from the library."""
        limits = self._wide_dim
        if limits is None:
            limits = self._wide_dim = (int(self._lib.aesmc_affine_wide_dim()), int(self._lib.aesmc_affine_wide_min_dim()),
                                       int(self._lib.aesmc_affine_wide_max_dim()))
        return limits

    def affine_wide_covers(self, source, weight, offset=None, scale=None):
        """Host-only test of what K17 / K18 (rows of 128 values) and K17g / K18g (every other width) assume about one
        location `offset + source @ weight.T`: source [B,K,din] float32 on the HIP device with 17 <= din <= 256, weight
        [dout,din] as an nn.Linear holds it with dout <= 256, offset None, [dout] or [B,dout], scale (if given) one value.
        (Maps of at most 16 x 16 are the item kernels': `affine_covers`.)"""
        if not (torch.is_tensor(weight) and weight.dim() == 2 and weight.dtype == torch.float32 and weight.is_cuda):
            return False
        _, smallest, largest = self._wide_limits()
        shape = tuple(source.shape)
        dout, din = weight.shape
        if len(shape) != 3 or shape[2] != din or source.dtype != torch.float32 or source.device != weight.device or \
                shape[0] * shape[1] == 0:
            return False
        if not (smallest <= din <= largest) or not (1 <= dout <= largest):
            return False
        if not weight.is_contiguous():
            return False
        if offset is not None:
            if not torch.is_tensor(offset) or offset.dtype != torch.float32 or offset.device != weight.device or \
                    tuple(offset.shape) not in ((dout,), (shape[0], dout)) or offset.stride(-1) != 1:
                return False
        if scale is not None and not (torch.is_tensor(scale) and scale.numel() == 1 and scale.dtype == torch.float32 and
                                      scale.device == weight.device):
            return False
        return True

    def affine_propagate_wide(self, x_src, eps, y_rows, transition, emission, proposal, scales, out_x, ancestors=None):
        """K17 + K18 (rows of 128 values) / K17g + K18g (any latent width from 17 to 256, any observation width up to 256,
        any K): a linear-Gaussian step on the fp32 matrix cores — the draw `loc_q(x_prev) + eps * s_q` into `out_x` (the C
        oracle's bits) and the step's log-weights [B,K] (its values to rounding), x_prev = x_src[b, ancestors[b,k]] when
        `ancestors` is given.
        `eps`: the noise [B,K,dx], or an `_philox.NoiseStream` — the reservation of the `normal_` call that did not
        happen: the launch then forms the noise itself (None when the shape does not allow it — anything but rows of 128
        values with K a multiple of 4 * threads / 128: the caller materialises it with `philox_normal`).
        None when the launch does not cover the operands (other extents, strided weights)."""
        if x_src.dtype != torch.float32 or x_src.dim() != 3:
            return None
        B, K, dx = x_src.shape
        wide, smallest, largest = self._wide_limits()
        if not (smallest <= dx <= largest) or B * K == 0 or not x_src.is_cuda:
            return None
        # the observation as K18 reads it: float32 [B, dy] on the latents' device (a float64 observation — torch.from_numpy
        # data against a float32 model — would be read as float32 bytes: declined, PyTorch's promotion applies instead)
        if not (torch.is_tensor(y_rows) and y_rows.dim() == 2 and y_rows.size(0) == B and
                y_rows.dtype == torch.float32 and y_rows.device == x_src.device):
            return None
        dy = y_rows.size(1)
        if not (1 <= dy <= largest):
            return None
        drawn = not torch.is_tensor(eps)      # an `_philox.NoiseStream`: the launch forms the noise itself
        if drawn:
            if eps.numel != x_src.numel():
                raise ValueError("aesmc_amd: affine_propagate_wide: the reservation does not match x_src")
            if dx != wide or dy != wide or K % 32 or eps.threads % wide or K % (4 * (eps.threads // wide)):
                return None
        else:
            self._expect(eps, x_src.shape, x_src, "affine_propagate_wide noise")
        for (weight, offset), scale, shape in zip((transition, emission, proposal), scales, ((dx, dx), (dy, dx), (dx, dx))):
            # (what affine_wide_covers tests, for callers that did not ask it)
            if not (torch.is_tensor(weight) and tuple(weight.shape) == shape and weight.is_contiguous() and
                    weight.dtype == torch.float32 and weight.device == x_src.device):
                return None
            if offset is not None and not (torch.is_tensor(offset) and offset.dtype == torch.float32 and
                                           offset.device == x_src.device and
                                           tuple(offset.shape) in ((shape[0],), (B, shape[0])) and offset.stride(-1) == 1):
                return None      # (rows / bases that are not 16-byte pieces: the launch moves them element by element)
            if not (torch.is_tensor(scale) and scale.numel() == 1 and scale.dtype == torch.float32 and
                    scale.device == x_src.device):
                return None
        self._check_out(out_x, (B, K, dx), x_src, "affine_propagate_wide")
        x_src = self._dense16(x_src)
        if not drawn:
            eps = self._dense16(eps)
        if out_x.data_ptr() == x_src.data_ptr() or (not drawn and out_x.data_ptr() == eps.data_ptr()):
            raise ValueError("aesmc_amd: affine_propagate_wide cannot write the draw over its inputs")
        ancestors = self._ancestors(x_src, ancestors, B, K, "affine_propagate_wide")
        if y_rows.stride(1) != 1 or y_rows.stride(0) % 4 or y_rows.data_ptr() % 16:
            y_rows = y_rows.contiguous()
        out = torch.empty((B, K), dtype=torch.float32, device=x_src.device)
        ws_bytes = int(self._lib.aesmc_affine_wide_workspace_bytes_for(B, K, dx, dy))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x_src.device)
        maps = [self._affine_map(*term, slot=slot) for slot, term in enumerate((transition, emission, proposal))]
        noise = (eps.seed, eps.offset, eps.threads, _ptr(eps.state)) if drawn else (0, 0, 256, 0)
        args = (_ptr(x_src), _ptr(ancestors), 0 if drawn else _ptr(eps), _ptr(y_rows), y_rows.stride(0)) + \
            self._map_args(maps, scales) + (_ptr(out_x), _ptr(out), _ptr(ws), ws_bytes, _ptr(self.flags(x_src.device)),
                                            B, K) + noise + (self._stream(x_src),)
        if not self._launch(x_src.device, self._lib.aesmc_affine_normal_propagate_wide, args,
                            lambda: 4 * (B * K * (3 * dx + 1) + y_rows.numel()) + (8 * B * K if ancestors is not None else 0),
                            (x_src, ancestors, eps, y_rows, out, out_x, ws, maps, scales), decline=True):
            return None
        return out

    def affine_initial_step(self, eps, loc_q, scale_q, loc_p, scale_p, y, weight, offset, scale_g, out_x):
        """K20: the first timestep of a run in one launch — `out_x[b,k,:] = loc_q + eps[k,b,:] * scale_q` (the reference's
        transposed `rsample((K,))`), the emission's location `offset + out_x @ weight.T` and the three Normal
        log-densities — with the bits of K6 + K8 + K5 (aesmc_affine_normal_initial_step).  `eps` [K,B,dx] contiguous;
        `loc_q`, `scale_q`, `loc_p`, `scale_p` views of [B,K,dx] and `y`, `scale_g` of [B,K,dy] whose particle stride is 0;
        `weight` [dy,dx] (any strides), `offset` None, [dy] or [B,dy].  Returns the log-weights [B,K], or None where the
        launch does not apply (nothing has been launched then)."""
        B, K, dx = out_x.shape
        if not (torch.is_tensor(eps) and eps.dtype == torch.float32 and eps.is_cuda and tuple(eps.shape) == (K, B, dx) and
                eps.is_contiguous() and out_x.dtype == torch.float32 and out_x.is_contiguous() and out_x.device == eps.device):
            return None
        if not (torch.is_tensor(weight) and weight.dim() == 2 and weight.size(1) == dx and weight.dtype == torch.float32 and
                weight.device == eps.device and 1 <= dx <= 16 and 1 <= weight.size(0) <= 16):
            return None
        dy = weight.size(0)
        if offset is not None and not (torch.is_tensor(offset) and offset.dtype == torch.float32 and
                                       offset.device == eps.device and tuple(offset.shape) in ((dy,), (B, dy))):
            return None
        views = []
        for view, extent in ((loc_q, dx), (scale_q, dx), (loc_p, dx), (scale_p, dx), (y, dy), (scale_g, dy)):
            if not (torch.is_tensor(view) and view.dtype == torch.float32 and view.device == eps.device and
                    tuple(view.shape) == (B, K, extent) and (K == 1 or view.stride(1) == 0)):
                return None
            views.append(_lib.View3(_ptr(view), view.stride(0), 0, view.stride(2)))
        out = torch.empty((B, K), dtype=torch.float32, device=eps.device)
        amap, held = self._affine_map(weight, offset)
        args = (_ptr(eps),) + tuple(ctypes.byref(v) for v in views[:5]) + (ctypes.byref(amap), ctypes.byref(views[5]),
                                                                            _ptr(out_x), _ptr(out), B, K, self._stream(eps))
        if not self._launch(eps.device, self._lib.aesmc_affine_normal_initial_step, args,
                            lambda: 4 * (2 * B * K * dx + B * K),
                            (eps, loc_q, scale_q, loc_p, scale_p, y, scale_g, out_x, out, views, amap, held), decline=True):
            return None
        return out

    def begin_evaluation(self):
        """Called once per `infer`: weight pairs built for an earlier evaluation are dropped (the weights may have been
        stepped in between; inside a hipGraph capture the rebuild must be part of the captured work; and the entry holds
        references to the weight tensors — with their autograd history, if they are computed per evaluation — which must
        not outlive the evaluation they belong to)."""
        self.evaluation += 1
        self._pairs = None

    def _build_pairs(self, maps, scales, device):
        """One launch: the interleaved pairs, with the three densities' constants behind them when `scales` is given
        (aesmc_affine_weight_pairs_scaled) — else their tag cleared (the propagating launch forms them itself)."""
        pairs = torch.empty(int(self._lib.aesmc_affine_weight_pairs_floats()), dtype=torch.float32, device=device)
        entry = self._lib.aesmc_affine_weight_pairs if scales is None else self._lib.aesmc_affine_weight_pairs_scaled
        self._launch(pairs.device, entry, self._map_args(maps, scales) + (_ptr(pairs), self._stream(pairs)))   # (not timed)
        return pairs

    # how often one evaluation may rebuild the pairs because the SCALES it was handed are other tensors than last time
    # (a model that computes them per timestep): after that the pairs carry no constants and fit any scales
    SCALED_PAIRS_REBUILDS = 2

    def _weight_pairs(self, maps, weights, device, scales=None):
        """The three maps' weights as interleaved pairs (aesmc_affine_weight_pairs[_scaled]) for the fused propagation
        launch: built by one small launch the first time an evaluation meets these weights, then reused by its other
        timesteps.  The entry keeps the weight (and scale) tensors alive for as long as it stands (until the next
        `begin_evaluation`), so a cached (address, version) can never be met again on a DIFFERENT tensor that the
        allocator placed where a freed one was.

        `scales` (three one-value float32 tensors): the densities' constants ride behind the pairs while the evaluation
        keeps handing in the SAME scale tensors, unchanged (`is` and `_version`: Python-number scales are cached device
        constants, parameters live as long as the model); other tensors rebuild — twice per evaluation at most, then
        the entry carries no constants."""
        w0, w1, w2 = weights
        if scales is not None and not all(torch.is_tensor(s) and s.dtype == torch.float32 and s.numel() == 1 and
                                          not s.is_inference() for s in scales):
            scales = None
        if any(w.is_inference() for w in weights):      # (no version counter to tell an in-place update by: never cached)
            return self._build_pairs(maps, scales, device)
        held = self._pairs
        key = (self.evaluation, w0._version, w1._version, w2._version)
        layout = None
        same = held is not None and held[0] == key and held[2] is w0 and held[3] is w1 and held[4] is w2
        # (the very tensors of this evaluation's last step, unchanged since: a model's next timestep)
        if not same and held is not None and held[0] == key:
            layout = tuple((w.data_ptr(), w.shape, w.stride()) for w in weights)
            same = held[5] == layout      # (new view objects of the same, still referenced, storage: `x @ W.t()` makes one per call)
        rebuilds = 0
        if same:
            for_scales = held[6]
            if for_scales is None:      # no constants behind these pairs: they fit any scales
                return held[1]
            if scales is not None and all(a is b for a, b in zip(for_scales[0], scales)) and \
                    for_scales[1] == tuple(s._version for s in scales):
                return held[1]
            rebuilds = held[7] + 1
            if rebuilds > self.SCALED_PAIRS_REBUILDS:
                scales = None
        if layout is None:
            layout = tuple((w.data_ptr(), w.shape, w.stride()) for w in weights)
        pairs = self._build_pairs(maps, scales, device)
        for_scales = None if scales is None else (tuple(scales), tuple(s._version for s in scales))
        self._pairs = (key, pairs, w0, w1, w2, layout, for_scales, rebuilds)
        return pairs

    def affine_propagate_drawn(self, x_src, noise, y_rows, transition, emission, proposal, scales, out_x,
                               ancestors=None):
        """K16: K15 with the resampling gather (`ancestors`, or None) AND the noise inside the launch — `noise`
        is an `_philox.NoiseStream`, the reservation of the `normal_` call that did not happen.  Returns the
        log-weights [B,K], or None when the launch does not cover the shape (the caller materialises the
        noise with `philox_normal` and takes `affine_propagate`)."""
        if x_src.dtype != torch.float32:
            return None
        B, K, dx = x_src.shape
        if B * K < self.DRAWN_MIN_PARTICLES:
            return None
        if noise.numel != B * K * dx:
            raise ValueError("aesmc_amd: affine_propagate_drawn: the reservation does not match x_src")
        self._check_out(out_x, (B, K, dx), x_src, "affine_propagate_drawn")
        x_src = self._dense16(x_src)
        if out_x.data_ptr() == x_src.data_ptr():
            raise ValueError("aesmc_amd: affine_propagate_drawn cannot write the draw over x_src")
        words = None
        if type(ancestors) is PackedAncestors:      # the item form reads the words as they are (4 B per particle)
            if ancestors.words.shape != (B, K) or ancestors.words.device != x_src.device:
                raise ValueError("aesmc_amd: affine_propagate_drawn ancestors must be [{}, {}] on {}".format(B, K, x_src.device))
            words = ancestors.words
        else:
            ancestors = self._ancestors(x_src, ancestors, B, K, "affine_propagate_drawn")
        y_rows = self._unit_rows(y_rows)
        out = torch.empty((B, K), dtype=x_src.dtype, device=x_src.device)
        maps = [self._affine_map(*term, slot=slot) for slot, term in enumerate((transition, emission, proposal))]
        pairs = None
        if self.WEIGHT_PAIRS and 2 <= dx <= 16:
            pairs = self._weight_pairs(maps, (transition[0], emission[0], proposal[0]), x_src.device,
                                       scales if self.SCALED_PAIRS else None)
        if words is not None:
            args = (_ptr(x_src), _ptr(words), _ptr(y_rows), y_rows.stride(0)) + self._map_args(maps, scales) + \
                (_ptr(out_x), _ptr(out), _ptr(self.flags(x_src.device)), B, K, noise.seed, noise.offset, noise.threads,
                 _ptr(noise.state), _ptr(pairs), self._stream(x_src))
            if self._launch(x_src.device, self._lib.aesmc_affine_normal_propagate_drawn_packed, args,
                            lambda: 4 * (B * K * (2 * dx + 1) + y_rows.numel()) + 8 * B * K,
                            (x_src, words, None, y_rows, out, out_x, maps, scales, pairs),
                            name="affine_normal_propagate_drawn", decline=True):
                return out
            ancestors = self._ancestors(x_src, ancestors, B, K, "affine_propagate_drawn")      # (another form: the int64 indices)
        args = (_ptr(x_src), _ptr(ancestors), _ptr(y_rows), y_rows.stride(0)) + self._map_args(maps, scales) + \
            (_ptr(out_x), _ptr(out), _ptr(self.flags(x_src.device)), B, K, noise.seed, noise.offset, noise.threads,
             _ptr(noise.state), _ptr(pairs), self._stream(x_src))
        if not self._launch(x_src.device, self._lib.aesmc_affine_normal_propagate_drawn_paired, args,
                            lambda: 4 * (B * K * (2 * dx + 1) + y_rows.numel()) + (8 * B * K if ancestors is not None else 0),
                            (x_src, ancestors, None, y_rows, out, out_x, maps, scales, pairs),
                            name="affine_normal_propagate_drawn", decline=True):
            return None
        return out

    def affine_logweight_covers(self, x_prev, x, y_rows, transition, emission, proposal, scales):
        """Host-only test of K10's preconditions; each of transition / emission / proposal is
        (weight, offset or None), y_rows the observation [B, dy], scales three one-value tensors."""
        if not (torch.is_tensor(x) and torch.is_tensor(x_prev) and torch.is_tensor(y_rows)):
            return False
        last = self._covers_last
        if last is not None and last[0] is transition[0] and last[1] is emission[0] and last[2] is proposal[0] and \
                last[3] is scales[0] and last[4] is scales[1] and last[5] is scales[2]:
            # the very parameter tensors of the step accepted last (a model's next timestep): what can differ are
            # the per-step operands — shapes, dtypes and devices of x_{t-1}, x_t, the observation and the offsets
            shape, dtype, device = last[6]
            weight = transition[0]
            if x.shape == shape and x_prev.shape == shape and x.dtype == dtype and x_prev.dtype == dtype and \
                    x.device == device and x_prev.device == device and weight.dtype == dtype and weight.device == device \
                    and y_rows.dtype == dtype and y_rows.device == device and y_rows.shape == last[7] and \
                    self._offsets_signature(transition[1], emission[1], proposal[1], dtype, device) == last[8]:
                return True
        if x_prev.shape != x.shape or x_prev.dtype != x.dtype or x_prev.device != x.device:
            return False
        if not (self.affine_covers(x_prev, *transition) and self.affine_covers(x, *emission) and
                self.affine_covers(x_prev, *proposal)):
            return False
        dx = x.size(2)
        if transition[0].size(0) != dx or proposal[0].size(0) != dx:
            return False
        if y_rows.dim() != 2 or y_rows.shape != (x.size(0), emission[0].size(0)) or \
                y_rows.dtype != x.dtype or y_rows.device != x.device:
            return False
        if not all(torch.is_tensor(s) and s.numel() == 1 and s.dtype == x.dtype and s.device == x.device
                   for s in scales):
            return False
        signature = self._offsets_signature(transition[1], emission[1], proposal[1], x.dtype, x.device)
        kept = (transition[0], emission[0], proposal[0]) + tuple(scales)
        if any(t.grad_fn is not None for t in kept):      # views with an autograd history are not kept (see _affine_map)
            self._covers_last = None
        elif signature is not None:
            self._covers_last = (transition[0], emission[0], proposal[0], scales[0], scales[1], scales[2],
                                 (x.shape, x.dtype, x.device), y_rows.shape, signature)
        return True

    @staticmethod
    def _offsets_signature(off_p, off_g, off_q, dtype, device):
        """Shapes of the three offsets (None where absent) when they are tensors of `dtype` on `device`, else None."""
        out = []
        for offset in (off_p, off_g, off_q):
            if offset is None:
                out.append(None)
            elif torch.is_tensor(offset) and offset.dtype == dtype and offset.device == device:
                out.append(offset.shape)
            else:
                return None
        return tuple(out)

    def affine_logweight(self, x_prev, x, y_rows, transition, emission, proposal, scales):
        """K10: the step's log-weight [B,K] with the three locations affine in the particles (see
        `affine_logweight_covers` for the operands)."""
        if not self.affine_logweight_covers(x_prev, x, y_rows, transition, emission, proposal, scales):
            raise ValueError("aesmc_amd: affine_logweight operands outside what kernel K10 covers")
        tag = _DTYPE_TAG[x.dtype]
        B, K, dx = x.shape
        x_prev, x = self._dense16(x_prev), self._dense16(x)
        y_rows = self._unit_rows(y_rows)
        out = torch.empty((B, K), dtype=x.dtype, device=x.device)
        maps = [self._affine_map(*term) for term in (transition, emission, proposal)]
        self._launch(x.device, self._lib.aesmc_affine_normal_logweight,
                     (tag, _ptr(x_prev), _ptr(x), _ptr(y_rows), y_rows.stride(0)) + self._map_args(maps, scales) +
                     (_ptr(out), B, K, self._stream(x)),
                     lambda: x.element_size() * (B * K * (2 * dx + 1) + y_rows.numel()),
                     (x_prev, x, y_rows, out, maps, scales))
        return out

    def particle_affine_backward(self, grad, x, weight, need_x=True, need_weight=True, need_offset=False):
        """K11, the adjoint of `offset + x @ weight.T` for grad [B,K,dout]: (grad_x = grad @ weight,
        grad_weight [dout,din] = sum over particles of grad (outer) x — on the matrix cores, summed in a
        fixed order —, grad_offset [B,dout] = sum over each row's particles of grad); entries not asked
        for are None."""
        if not (need_x or need_weight or need_offset):
            return None, None, None
        if not self.affine_covers(x, weight) or grad.shape != x.shape[:2] + (weight.size(0),) or \
                grad.dtype != x.dtype or grad.device != x.device:
            raise ValueError("aesmc_amd: particle_affine_backward operands outside what kernel K11 covers")
        tag = _DTYPE_TAG[x.dtype]
        B, K, din = x.shape
        dout = weight.size(0)
        grad, x = self._dense16(grad), self._dense16(x)
        in_kernel_offset = need_offset and (256 - 1) // K + 2 <= 8      # the kernel's row table: >= ~43 particles per row
        gx = torch.empty_like(x) if need_x else None
        gw = torch.empty((dout, din), dtype=x.dtype, device=x.device) if need_weight else None
        goff = torch.empty((B, dout), dtype=x.dtype, device=x.device) if in_kernel_offset else None
        reduces = need_weight or in_kernel_offset
        ws_bytes = int(self._lib.aesmc_affine_backward_workspace_bytes(tag, B, K)) if reduces else 0
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device) if ws_bytes else None
        amap, keep = self._affine_map(weight, None)
        entry = self._lib.aesmc_particle_affine_backward
        args = (tag, _ptr(grad), _ptr(x), ctypes.byref(amap), _ptr(gx), _ptr(gw), _ptr(goff), _ptr(ws), ws_bytes,
                B, K, self._stream(x))
        nbytes = lambda: x.element_size() * B * K * (dout + (din if need_weight else 0) + (din if need_x else 0))
        if not self._launch(x.device, entry, args, nbytes, (grad, x, gx, gw, goff, ws, amap, keep),
                            decline=goff is not None):
            goff = None     # the row sums do not fit this shape: the caller's reduction instead
            self._launch(x.device, entry, args[:6] + (0,) + args[7:], nbytes, (grad, x, gx, gw, goff, ws, amap, keep))
        if need_offset and goff is None:
            goff = grad.sum(dim=1)
        return gx, gw, goff

    def outer_sum(self, g, x):
        """sum over all particles of g[b,k,:] (outer) x[b,k,:] -> [dout, din]: the weight gradient of an
        affine location (K11 without the input gradient).  The weight's values are not read."""
        placeholder = torch.empty((g.size(2), x.size(2)), dtype=x.dtype, device=x.device)
        return self.particle_affine_backward(g, x, placeholder, need_x=False, need_weight=True)[1]

    @staticmethod
    def _affine_grad_buffers(need, offsets, dx, dy, dtype, device, B=None, sums=True):
        """The optional outputs of K12 / K14 / the collect in `aesmc_affine_logweight_grads` order after the dense ones:
        (grad_A, grad_C, grad_Q, the three scales' [3], then the three locations' gradients summed over each batch row's
        particles [B,dx] / [B,dy] / [B,dx]), None where `need` does not ask for one (`B` None: no row sums; `sums` false:
        no weight or scale sums — a deferring K14 leaves those as records)."""
        off_p, off_g, off_q = offsets
        make = lambda shape, wanted: torch.empty(shape, dtype=dtype, device=device) if wanted else None
        rows = B is not None
        rows_p = make((B, dx), rows and need[4] and off_p is not None)
        rows_g = make((B, dy), rows and ((need[6] and off_g is not None) or need[2]))
        rows_q = make((B, dx), rows and need[8] and off_q is not None)
        gA, gC, gQ = make((dx, dx), sums and need[3]), make((dy, dx), sums and need[5]), make((dx, dx), sums and need[7])
        gscales = make((3,), sums and (need[9] or need[10] or need[11]))
        return gA, gC, gQ, gscales, rows_p, rows_g, rows_q

    @staticmethod
    def _affine_grad_slots(g_prev, g_x, buffers, need, offsets, scales):
        """The 12-slot gradient list (x_prev, x, y_rows, A, off_p, C, off_g, Q, off_q, s_p, s_g, s_q) from the dense
        gradients and `_affine_grad_buffers`: y's is minus the emission's row sums, an offset's is its location's row sums
        (all rows added for a shared [d] offset)."""
        gA, gC, gQ, gscales, rows_p, rows_g, rows_q = buffers
        off_p, off_g, off_q = offsets
        fold = lambda rows, off: rows if off.dim() == 2 else rows.sum(dim=0)     # a shared [d] offset: all rows
        grads = [g_prev, g_x, None, gA, None, gC, None, gQ, None, None, None, None]
        if need[2] and rows_g is not None:
            grads[2] = -rows_g
        if rows_p is not None:
            grads[4] = fold(rows_p, off_p)
        if need[6] and off_g is not None and rows_g is not None:
            grads[6] = fold(rows_g, off_g)
        if rows_q is not None:
            grads[8] = fold(rows_q, off_q)
        for slot, s in ((9, scales[0]), (10, scales[1]), (11, scales[2])):
            if need[slot] and gscales is not None:
                grads[slot] = gscales[slot - 9].reshape(s.shape)
        return grads

    def affine_logweight_backward(self, x_prev, x, y_rows, transition, emission, proposal, scales, need,
                                  grad_lw=None, lw=None, lse=None, grad_lse=None):
        """K12: gradients of `affine_logweight` with respect to its twelve operands, in the order
        (x_prev, x, y_rows, A, off_p, C, off_g, Q, off_q, s_p, s_g, s_q); None where `need[i]` is false
        or the operand is absent.  The incoming gradient is `grad_lw` [B,K] and / or K1's softmax term
        grad_lse[b] * exp(lw - lse[b]) formed in place (`lw`, `lse`, `grad_lse`).  One pass over x_prev
        and x; the weight gradients are summed on the matrix cores in a fixed order."""
        if not self.affine_logweight_covers(x_prev, x, y_rows, transition, emission, proposal, scales):
            raise ValueError("aesmc_amd: affine_logweight_backward operands outside what kernel K12 covers")
        offsets = (transition[1], emission[1], proposal[1])
        tag = _DTYPE_TAG[x.dtype]
        B, K, dx = x.shape
        dy = y_rows.size(1)
        fused_lse = grad_lse is not None
        if fused_lse:
            lw, lse, grad_lse = lw.contiguous(), lse.contiguous(), grad_lse.contiguous()
            self._expect(lw, (B, K), x, "lw")
            self._expect(lse, (B,), x, "lse")
            self._expect(grad_lse, (B,), x, "grad_lse")
        if grad_lw is not None:
            grad_lw = grad_lw.contiguous()
            self._expect(grad_lw, (B, K), x, "grad_lw")
        elif not fused_lse:
            raise ValueError("aesmc_amd: affine_logweight_backward needs grad_lw or (lw, lse, grad_lse)")
        x_prev, x = self._dense16(x_prev), self._dense16(x)
        y_rows = self._unit_rows(y_rows)
        make = lambda wanted: torch.empty((B, K, dx), dtype=x.dtype, device=x.device) if wanted else None
        gx_prev, gx = make(need[0]), make(need[1])
        sums = self._affine_grad_buffers(need, offsets, dx, dy, x.dtype, x.device, B=B)
        ws_bytes = int(self._lib.aesmc_affine_backward_workspace_bytes(tag, B, K))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device)
        outs = _lib.AffineLogweightGrads(_ptr(gx_prev), _ptr(gx), 0, 0, 0, *map(_ptr, sums))
        maps = [self._affine_map(*term) for term in (transition, emission, proposal)]
        args = (tag, _ptr(x_prev), _ptr(x), _ptr(y_rows), y_rows.stride(0)) + self._map_args(maps, scales) + \
            (_ptr(lw) if fused_lse else 0, _ptr(lse) if fused_lse else 0, _ptr(grad_lse) if fused_lse else 0,
             _ptr(grad_lw), ctypes.byref(outs), _ptr(ws), ws_bytes, B, K, self._stream(x))
        if not self._launch(x.device, self._lib.aesmc_affine_normal_logweight_backward, args,
                            lambda: x.element_size() * (B * K * (2 * dx + 1)) +
                            sum(t.numel() * t.element_size() for t in (gx_prev, gx) if t is not None),
                            (x_prev, x, y_rows, lw, lse, grad_lse, grad_lw, outs, ws, maps, scales) + sums + (gx_prev, gx),
                            decline=True):
            # too few particles per batch row for the fused kernel's row table
            return self.affine_logweight_backward_unfused(
                x_prev, x, y_rows, transition, emission, proposal, scales, need, grad_lw=grad_lw,
                lw=lw if fused_lse else None, lse=lse if fused_lse else None,
                grad_lse=grad_lse if fused_lse else None)
        return self._affine_grad_slots(gx_prev, gx, sums, need, offsets, scales)

    def affine_logweight_backward_unfused(self, x_prev, x, y_rows, transition, emission, proposal, scales, need,
                                          grad_lw=None, lw=None, lse=None, grad_lse=None):
        """The same gradients by the route K12 replaces — K8 x 3 to materialise the locations, K5's
        backward, K8 on the transposed weights, K11's outer sums — kept as the cross-check of K12."""
        (A, off_p), (C, off_g), (Q, off_q) = transition, emission, proposal
        s_p, s_g, s_q = scales
        B, K, dx = x.shape
        dy = y_rows.size(1)
        loc_p = self.particle_affine(x_prev, A, off_p)
        loc_g = self.particle_affine(x, C, off_g)
        loc_q = self.particle_affine(x_prev, Q, off_q)
        y_expanded = y_rows.unsqueeze(1).expand(B, K, dy)
        want = [True, True, bool(need[9]), bool(need[2]), True, bool(need[10]), True, bool(need[11])]
        outs = self.normal_logweight_backward(x, loc_p, s_p.expand_as(loc_p), y_expanded, loc_g,
                                              s_g.expand_as(loc_g), loc_q, s_q.expand_as(loc_q), grad_lw, want,
                                              lw=lw, lse=lse, grad_lse=grad_lse)
        if outs is None:
            raise RuntimeError("aesmc_amd: K5's backward declined operands of an affine step")
        gx, g_loc_p, g_sp, g_y, g_loc_g, g_sg, g_loc_q, g_sq = outs
        fold = lambda g, off: None if off is None else (g.sum(dim=1) if off.dim() == 2 else g.sum(dim=(0, 1)))
        grads = [None] * 12
        if need[0]:
            grads[0] = self.particle_affine(g_loc_p, A.t(), None, g_loc_q, Q.t())
        if need[1]:
            grads[1] = self.particle_affine(g_loc_g, C.t(), base=gx)
        if need[2]:
            grads[2] = g_y.sum(dim=1)
        if need[3]:
            grads[3] = self.outer_sum(g_loc_p, x_prev)
        if need[4] and off_p is not None:
            grads[4] = fold(g_loc_p, off_p)
        if need[5]:
            grads[5] = self.outer_sum(g_loc_g, x)
        if need[6] and off_g is not None:
            grads[6] = fold(g_loc_g, off_g)
        if need[7]:
            grads[7] = self.outer_sum(g_loc_q, x_prev)
        if need[8] and off_q is not None:
            grads[8] = fold(g_loc_q, off_q)
        for slot, g, s in ((9, g_sp, s_p), (10, g_sg, s_g), (11, g_sq, s_q)):
            if need[slot]:
                grads[slot] = g.sum().reshape(s.shape)
        return grads

    # ---- K14: the whole backward of a step whose x_t is the proposal's reparameterised draw ------
    def affine_step_backward(self, x_prev, x, y_rows, transition, emission, proposal, scales, need, lw, lse,
                             grad_lse=None, grad_x=None, grad_lw=None, ancestors=None, child_grad=None, child_end=None,
                             chain=None):
        """K14: gradients of one SMC step (log-weights `lw` of K10, their row log-sum-exp `lse`) whose x IS the
        draw  loc_q(x_prev) + s_q eps  of K9 from the same proposal operands, with respect to
        (x_prev, x, y_rows, A, off_p, C, off_g, Q, off_q, s_p, s_g, s_q) — x's own slot is always None: the
        gradient `grad_x` that arrives at x from later steps and the step's own gradient at x travel on
        through the draw inside the kernel (K12 + K11 + the accumulations between them, one pass).
        `chain` (a dict, only through ancestors): {"carry": (workspace, records[, pairs address, pairs' holder]) of the step run before this one with the
        SAME A, C, Q and scales, or None; "defer": leave this step's sums for those parameters as records}.  A
        deferring call returns None in their slots and sets chain["left"] = (workspace, records) for the next call
        to carry; a carrying call's gradients for them include everything carried.  Where the kernel declines the
        shape, what was carried is collected and added here and nothing is left (chain["left"] = None)."""
        if chain is not None:
            chain["left"] = None
            if ancestors is None:
                raise ValueError("aesmc_amd: affine_step_backward chains the weights' gradients only through ancestors")
        # `ancestors` / `child_end` as `PackedAncestors` (this step's resampling, the next step's): the rows form of the
        # kernel reads the words as they are; any other form, and any mix with plain tensors, gets them unpacked
        words = child_words = None
        if type(ancestors) is PackedAncestors and (child_grad is None or type(child_end) is PackedAncestors) and \
                x.dim() == 3 and x.size(2) <= self.affine_max_dim and x.dtype == torch.float32 and \
                ancestors.words.shape == x.shape[:2] and ancestors.words.device == x.device:
            words = ancestors.words
            if child_grad is not None:
                if child_end.words.shape != x.shape[:2] or child_end.words.device != x.device or not child_end.has_ranges:
                    raise ValueError("aesmc_amd: affine_step_backward child_end must hold the ranges of [{}, {}] particles on "
                                     "{}".format(x.size(0), x.size(1), x.device))
                child_words = child_end.words
        else:
            ancestors = as_index(ancestors)
            if type(child_end) is PackedAncestors:
                child_end = child_end.child_end()
        if x.dim() == 3 and x.size(2) > self.affine_max_dim:
            if chain is not None or child_grad is not None:
                raise ValueError("aesmc_amd: a wide step's backward takes the summed gradient (no children ranges, no chain)")
            return self.affine_step_backward_wide(x_prev, x, y_rows, transition, emission, proposal, scales, need, lw, lse,
                                                  grad_lse=grad_lse, grad_x=grad_x, grad_lw=grad_lw, ancestors=ancestors)
        if not self.affine_logweight_covers(x_prev, x, y_rows, transition, emission, proposal, scales):
            raise ValueError("aesmc_amd: affine_step_backward operands outside what kernel K14 covers")
        if need[1]:
            raise ValueError("aesmc_amd: affine_step_backward: x is the proposal's draw and has no gradient slot")
        offsets = (transition[1], emission[1], proposal[1])
        tag = _DTYPE_TAG[x.dtype]
        B, K, dx = x.shape
        dy = y_rows.size(1)
        fused_lse = grad_lse is not None
        if fused_lse:
            lw, lse, grad_lse = lw.contiguous(), lse.contiguous(), grad_lse.contiguous()
            self._expect(lw, (B, K), x, "lw")
            self._expect(lse, (B,), x, "lse")
            self._expect(grad_lse, (B,), x, "grad_lse")
        if grad_lw is not None:
            grad_lw = grad_lw.contiguous()
            self._expect(grad_lw, (B, K), x, "grad_lw")
        if grad_x is not None:
            grad_x = self._dense16(grad_x)
            self._expect(grad_x, (B, K, dx), x, "grad_x")
        if not fused_lse and grad_lw is None and grad_x is None and child_grad is None:
            raise ValueError("aesmc_amd: affine_step_backward needs a gradient: (lw, lse, grad_lse), grad_lw or grad_x")
        if child_grad is not None:
            # the NEXT step's gradient of the rows it resampled from x (one row per child) and its children ranges: the
            # kernel sums each particle's children itself — torch.gather's backward, where it is consumed
            if ancestors is None:
                raise ValueError("aesmc_amd: affine_step_backward folds the children's gradient only through ancestors")
            self._expect(child_grad, (B, K, dx), x, "child_grad")
            child_grad = self._dense16(child_grad)
            if child_words is None:
                if child_end is None or child_end.shape != (B, K) or child_end.dtype != torch.int32 or \
                        child_end.device != x.device:
                    raise ValueError("aesmc_amd: affine_step_backward child_end must be int32 [{}, {}] on {}".format(B, K, x.device))
                child_end = child_end.contiguous()
        # `x_prev` is the un-resampled latent when `ancestors` is given: the kernel fetches x_prev[b, ancestors[b,k]]
        # itself and slot 0 of the result is the gradient of those RESAMPLED rows (the caller sums children into ancestors)
        if words is None:
            ancestors = self._ancestors(x_prev, ancestors, B, K, "affine_step_backward")
        x_prev, x = self._dense16(x_prev), self._dense16(x)
        y_rows = self._unit_rows(y_rows)
        gx_prev = torch.empty((B, K, dx), dtype=x.dtype, device=x.device) if need[0] else None
        carry = chain["carry"] if chain is not None else None
        defer = chain is not None and bool(chain["defer"])
        sums = self._affine_grad_buffers(need, offsets, dx, dy, x.dtype, x.device, B=B, sums=not defer)
        ws_bytes = int(self._lib.aesmc_affine_backward_workspace_bytes(tag, B, K))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device)
        outs = _lib.AffineLogweightGrads(_ptr(gx_prev), 0, 0, 0, 0, *map(_ptr, sums))
        maps = [self._affine_map(*term) for term in (transition, emission, proposal)]
        middle = (_ptr(x), _ptr(y_rows), y_rows.stride(0)) + self._map_args(maps, scales) + \
            (_ptr(lw) if fused_lse else 0, _ptr(lse) if fused_lse else 0, _ptr(grad_lse) if fused_lse else 0,
             _ptr(grad_lw), _ptr(grad_x))
        tail = (ctypes.byref(outs), _ptr(ws), ws_bytes)
        link = None
        if chain is not None:
            # (carry[2], carry[3]: where the run's interleaved weight pairs lie and the workspace that holds them — built by
            #  the run's first call, handed on from step to step instead of one small launch per step)
            pairs_in = carry[2] if carry is not None and len(carry) > 2 and carry[2] else 0
            link = _lib.AffineChain(_ptr(carry[0]) if carry is not None else 0, carry[1] if carry is not None else 0,
                                    (2 if (need[9] or need[10] or need[11]) else 1) if defer else 0, 0, pairs_in, 0)
        esz = x.element_size()
        if words is not None:
            args = (tag, _ptr(x_prev), _ptr(words)) + middle + (_ptr(child_grad), _ptr(child_words)) + tail + \
                (_ptr(self.flags(x.device)), ctypes.byref(link) if link is not None else None, B, K, self._stream(x))
            if self._launch(x.device, self._lib.aesmc_affine_step_backward_packed, args,
                            lambda: esz * B * K * (2 * dx + 1 + (dx if grad_x is not None else 0) + (dx if gx_prev is not None else 0)) +
                            8 * B * K + (esz * B * K * dx + 4 * B * K if child_grad is not None else 0),
                            (x_prev, words, x, y_rows, lw, lse, grad_lse, grad_lw, grad_x, child_grad, child_words, outs,
                             ws, maps, scales) + sums + (gx_prev, link, carry), name="affine_step_backward_resampled",
                            decline=True):
                if defer:
                    handed_on = carry is not None and len(carry) > 2 and carry[2] and link.pairs_out == carry[2]
                    chain["left"] = (ws, int(link.records), link.pairs_out or 0, carry[3] if handed_on else ws)
                return self._affine_grad_slots(gx_prev, None, sums, need, offsets, scales)
            # (not a shape of the rows form: the two arrays, one unpack launch per handle, and the entry that takes them)
            ancestors = self._ancestors(x_prev, ancestors, B, K, "affine_step_backward")
            if child_grad is not None:
                child_end = child_end.child_end()
        if ancestors is not None:
            entry = self._lib.aesmc_affine_step_backward_resampled
            args = (tag, _ptr(x_prev), _ptr(ancestors)) + middle + (_ptr(child_grad), _ptr(child_end)) + tail + \
                (_ptr(self.flags(x.device)), ctypes.byref(link) if link is not None else None, B, K, self._stream(x))
        else:
            entry = self._lib.aesmc_affine_step_backward
            args = (tag, _ptr(x_prev)) + middle + tail + (B, K, self._stream(x))
        nbytes = lambda: esz * B * K * (2 * dx + 1 + (dx if grad_x is not None else 0) + (dx if gx_prev is not None else 0)) + \
            (8 * B * K if ancestors is not None else 0) + (esz * B * K * dx + 4 * B * K if child_grad is not None else 0)
        if not self._launch(x.device, entry, args, nbytes,
                            (x_prev, ancestors, x, y_rows, lw, lse, grad_lse, grad_lw, grad_x, child_grad, child_end, outs,
                             ws, maps, scales) + sums + (gx_prev, link, carry), decline=True):
            if child_grad is not None:      # the unfused route takes the summed gradient as a tensor
                summed = self.gather_backward_ranges(child_grad, child_end)
                grad_x, child_grad, child_end = (summed if grad_x is None else grad_x + summed), None, None
            if ancestors is not None:       # the unfused route wants the resampled rows as a tensor
                x_prev, ancestors = self.gather(x_prev, ancestors), None
            # too few particles per batch row for the fused kernel's row table
            grads = self.affine_step_backward_unfused(
                x_prev, x, y_rows, transition, emission, proposal, scales, need, lw if fused_lse else None,
                lse if fused_lse else None, grad_lse=grad_lse if fused_lse else None, grad_x=grad_x,
                grad_lw=grad_lw)
            if carry is not None:      # what the steps before left: finished here, added to this step's own
                carried = self.affine_backward_collect(carry, x.dtype, x.device, dx, dy, need, scales)
                for slot, value in enumerate(carried):
                    if value is not None:
                        grads[slot] = value if grads[slot] is None else grads[slot] + value
            return grads
        if defer:
            handed_on = carry is not None and len(carry) > 2 and carry[2] and link.pairs_out == carry[2]
            chain["left"] = (ws, int(link.records), link.pairs_out or 0, carry[3] if handed_on else ws)
        return self._affine_grad_slots(gx_prev, None, sums, need, offsets, scales)

    @property
    def wide_dim(self):
        return self._wide_limits()[0]

    @property
    def wide_adjoint_tile(self):
        tile = getattr(self, "_wide_adjoint_tile", None)
        if tile is None:
            tile = self._wide_adjoint_tile = int(self._lib.aesmc_wide_adjoint_tile())
        return tile

    def _wide_adjoint_covers(self, u, weight, scale):
        """Do aesmc_wide_adjoint_scale / _merge take these operands (rows of 128 float32 values, dense, whole tiles)?"""
        return (u.dtype == torch.float32 and u.dim() == 3 and u.size(2) == self.wide_dim and u.is_contiguous() and
                u.size(1) % self.wide_adjoint_tile == 0 and u.numel() > 0 and weight.dtype == torch.float32 and
                weight.shape == u.shape[:2] and weight.is_contiguous() and scale.dtype == torch.float32 and
                scale.numel() == 1 and u.data_ptr() % 16 == 0)

    def wide_adjoint_scale(self, u, weight, scale, want_sq, want_rows, base=None):
        """`u` [B,K,128] (a residual d — or, `base` [B,128] given, the location, d = base[b] - u — overwritten by the
        location's adjoint weight d / scale^2) -> (sum_j d_j^2 [B,K] or None, the adjoint summed over each batch row's
        particles [B,128] or None): aesmc_wide_adjoint_scale."""
        B, K, d = u.shape
        sq = torch.empty((B, K), dtype=torch.float32, device=u.device) if want_sq else None
        tiles = K // self.wide_adjoint_tile
        rows = torch.empty((B, tiles, d), dtype=torch.float32, device=u.device) if want_rows else None
        self._launch(u.device, self._lib.aesmc_wide_adjoint_scale,
                     (_ptr(u), _ptr(weight), _ptr(scale), _ptr(base), base.stride(0) if base is not None else 0, _ptr(sq),
                      _ptr(rows), B, K, self._stream(u)),
                     lambda: 8 * u.numel(), (u, weight, scale, sq, rows, base))
        return sq, (rows.sum(1) if rows is not None else None)

    def wide_adjoint_merge(self, u_p, at_x, weight, scale, want_sq, want_rows_p, want_rows_x, value=None, base=None,
                           add=None):
        """The transition's residual d in `u_p` (or, `value` [B,K,128] given, its location: d = (value - base[b]) - u_p, base
        [B,128] or None) and the gradient arriving at x_t in `at_x` (plus `add`, if given), both [B,K,128] and overwritten:
        u_p <- weight d / scale^2, at_x <- (add + at_x) - u_p; returns (sum_j d_j^2 [B,K], u_p's and at_x's sums over each batch row's particles
        [B,128]), None where not wanted: aesmc_wide_adjoint_merge."""
        B, K, d = u_p.shape
        tiles = K // self.wide_adjoint_tile
        sq = torch.empty((B, K), dtype=torch.float32, device=u_p.device) if want_sq else None
        rows_p = torch.empty((B, tiles, d), dtype=torch.float32, device=u_p.device) if want_rows_p else None
        rows_x = torch.empty((B, tiles, d), dtype=torch.float32, device=u_p.device) if want_rows_x else None
        self._launch(u_p.device, self._lib.aesmc_wide_adjoint_merge,
                     (_ptr(u_p), _ptr(at_x), _ptr(weight), _ptr(scale), _ptr(value), _ptr(base),
                      base.stride(0) if base is not None else 0, _ptr(add), _ptr(sq), _ptr(rows_p), _ptr(rows_x), B, K,
                      self._stream(u_p)),
                     lambda: 16 * u_p.numel(), (u_p, at_x, weight, scale, sq, rows_p, rows_x, value, base, add))
        return sq, (rows_p.sum(1) if rows_p is not None else None), (rows_x.sum(1) if rows_x is not None else None)

    def affine_step_backward_wide(self, x_prev, x, y_rows, transition, emission, proposal, scales, need, lw, lse,
                                  grad_lse=None, grad_x=None, grad_lw=None, ancestors=None):
        """`affine_step_backward` for rows wider than the fused kernels take (BASELINE.json configs[4]: 128 values): the
        same twelve gradients, RECOMPUTED from what the forward launches (K17 / K18) left — x_{t-1}, the ancestors, x_t,
        the log-weights — instead of retained: the step keeps no location, no noise and no resampled latent for its
        backward (three [B,K,128] tensors per timestep in the GEMM route: what made training at this extent outgrow HBM).
        The adjoint's contractions — three locations, three transposed maps, three sums of outer products over the
        particles — are [B K, 128] x [128, 128] products on the matrix cores through the GEMM library; the element-wise
        parts between them are PyTorch's.  Reference: autograd of aesmc/state.py:114-155, :179 and
        aesmc/inference.py:108-130 for one timestep."""
        (A, off_p), (C, off_g), (Q, off_q) = transition, emission, proposal
        s_p, s_g, s_q = scales
        B, K, dx = x.shape
        dy = y_rows.size(1)
        with torch.no_grad():
            moved = x_prev if ancestors is None else self.gather(x_prev, ancestors)      # x_{t-1}[b, ancestors[b, k]]
            weight = None
            if grad_lse is not None:
                weight = grad_lse.unsqueeze(1) * torch.exp(lw - lse.unsqueeze(1))           # d L / d lw through the row lse
            if grad_lw is not None:
                weight = grad_lw if weight is None else weight + grad_lw
            # residual = base - source @ W.T with the map's offset folded into `base` ([B,1,d'] broadcast over the
            # particles, or the full [B,K,d'] tensor): ONE pass — the GEMM's epilogue — instead of a product, an offset add
            # and a subtraction
            def residual(base, source, W, offset):
                if offset is not None:
                    base = base - (offset.unsqueeze(1) if offset.dim() == 2 else offset)
                return torch.baddbmm(base, source, W.t().unsqueeze(0).expand(B, -1, -1), beta=1, alpha=-1)
            # sum over the particles of u ⊗ v: [d', N] x [N, d] with N = B K in the millions is a shape the GEMM library
            # picks poor tiles for (0.8 - 0.9 ms at N = 2^20); as a batch of N / 4096 products of depth 4096, summed: ~0.4 ms
            def outer_sum(u, v):
                n = B * K
                depth = 4096 if n % 4096 == 0 and n > 4096 else n
                parts = torch.bmm(u.reshape(n // depth, depth, u.size(2)).transpose(1, 2), v.reshape(n // depth, depth, v.size(2)))
                return parts.sum(0) if parts.size(0) > 1 else parts[0]
            rows = lambda u, off: u.sum(1) if off.dim() == 2 else u.sum((0, 1))
            incoming = grad_x      # what arrives at x_t from later steps
            grads = [None] * 12
            at_prev = None
            rows_x = None
            if weight is not None:
                g = weight.unsqueeze(2)
                # emission: u_g = g (y - loc_g) / s_g^2 — its gradient reaches C, its offset, y, s_g and x_t (C^T u_g)
                weight = weight.contiguous()
                want_rows_g = (need[6] and off_g is not None) or need[2]
                fused = dx == dy and x.is_contiguous() and moved.is_contiguous() and \
                    self._wide_adjoint_covers(x, weight, s_g) and self._wide_adjoint_covers(x, weight, s_p)
                rows_g = None
                if fused:
                    # the location by a plain product, then ONE pass (K19): d = (y - offset)[b] - location formed there (no
                    # [B,K,128] copy of the broadcast row for an epilogue to start from), the adjoint in place, sum_j d_j^2
                    # per particle, the rows' sums
                    base_g = y_rows if off_g is None else y_rows - off_g
                    base_g = base_g.contiguous()
                    u_g = torch.matmul(x, C.t())
                    sq_g, rows_g = self.wide_adjoint_scale(u_g, weight, s_g, need[10], want_rows_g, base=base_g)
                    if need[10]:
                        grads[10] = (weight * (sq_g / s_g ** 3 - dy / s_g)).sum().reshape(s_g.shape)
                else:
                    u_g = residual(y_rows.unsqueeze(1), x, C, off_g)
                    if need[10]:
                        grads[10] = (weight * (u_g.square().sum(2) / s_g ** 3 - dy / s_g)).sum().reshape(s_g.shape)
                    u_g.mul_(g / (s_g * s_g))
                if need[5]:
                    grads[5] = outer_sum(u_g, x)
                if want_rows_g:
                    if rows_g is None:
                        rows_g = u_g.sum(1)
                    if need[6] and off_g is not None:
                        grads[6] = rows_g if off_g.dim() == 2 else rows_g.sum(0)
                    if need[2]:
                        grads[2] = -rows_g
                # what arrives at x_t: later steps' gradient + C^T u_g - u_p — in K19's one pass where it runs, else
                # accumulated in the products' epilogues
                later = None
                if fused and incoming is not None and incoming.is_contiguous() and incoming.dtype == torch.float32 and \
                        incoming.data_ptr() % 16 == 0:
                    later, at_x = incoming, torch.matmul(u_g, C)
                else:
                    at_x = torch.matmul(u_g, C) if incoming is None else \
                        torch.baddbmm(incoming, u_g, C.unsqueeze(0).expand(B, -1, -1))
                del u_g
                # transition: u_p = g (x_t - loc_p) / s_p^2 — reaches A, its offset, s_p, x_{t-1} (A^T u_p) and x_t (- u_p)
                rows_x = None
                if fused and at_x.is_contiguous():
                    # the location by a plain product, then one pass over it, x_t and at_x (K19): d = (x_t - offset) -
                    # location, u_p and at_x in place, sum_j d_j^2, both tensors' row sums
                    u_p = torch.matmul(moved, A.t())
                    sq_p, rows_p, rows_x = self.wide_adjoint_merge(
                        u_p, at_x, weight, s_p, need[9], need[4] and off_p is not None, need[8] and off_q is not None,
                        value=x, base=None if off_p is None else (off_p if off_p.dim() == 2 else off_p.unsqueeze(0).expand(B, -1)).contiguous(),
                        add=later)
                    if need[9]:
                        grads[9] = (weight * (sq_p / s_p ** 3 - dx / s_p)).sum().reshape(s_p.shape)
                    if need[4] and off_p is not None:
                        grads[4] = rows_p if off_p.dim() == 2 else rows_p.sum(0)
                else:
                    if later is not None:
                        at_x.add_(later)
                    u_p = residual(x, moved, A, off_p)
                    if need[9]:
                        grads[9] = (weight * (u_p.square().sum(2) / s_p ** 3 - dx / s_p)).sum().reshape(s_p.shape)
                    u_p.mul_(g / (s_p * s_p))
                    at_x.sub_(u_p)
                    if need[4] and off_p is not None:
                        grads[4] = rows(u_p, off_p)
                if need[3]:
                    grads[3] = outer_sum(u_p, moved)
                if need[0]:
                    at_prev = torch.matmul(u_p, A)
                del u_p
                incoming = at_x
            # the draw x_t = loc_q(x_{t-1}) + s_q eps carries everything that arrived at x_t to Q, its offset, s_q, x_{t-1}
            if incoming is not None:
                if need[7]:
                    grads[7] = outer_sum(incoming, moved)
                if need[8] and off_q is not None:
                    if weight is not None and rows_x is not None:
                        grads[8] = rows_x if off_q.dim() == 2 else rows_x.sum(0)
                    else:
                        grads[8] = rows(incoming, off_q)
                if need[11]:
                    noise_times_scale = residual(x, moved, Q, off_q)       # s_q eps
                    value = (incoming * noise_times_scale).sum() / s_q
                    if weight is not None:
                        value = value + weight.sum() * (dx / s_q)      # - d log q / d s_q = + d / s_q per particle
                    grads[11] = value.reshape(s_q.shape)
                if need[0]:
                    # (at_prev is this function's own product: accumulated in place — an out-of-place baddbmm copies it first)
                    at_prev = torch.matmul(incoming, Q) if at_prev is None else \
                        at_prev.baddbmm_(incoming, Q.unsqueeze(0).expand(B, -1, -1))
            elif need[11] and weight is not None:
                grads[11] = (weight.sum() * (dx / s_q)).reshape(s_q.shape)
            if need[0]:
                grads[0] = at_prev if at_prev is not None else torch.zeros_like(x)
        return grads

    def affine_backward_collect(self, left, dtype, device, dx, dy, need, scales):
        """The weights' and scales' gradients (a 12-slot list like affine_step_backward's, None elsewhere) out of the
        records a deferring K14 call left — `left` = its chain["left"] — when no later call carried them on."""
        ws, records = left[0], left[1]      # (+ where the run's weight pairs lie and their holder: not needed here)
        sums = self._affine_grad_buffers(need, (None, None, None), dx, dy, dtype, device)
        outs = _lib.AffineLogweightGrads(0, 0, 0, 0, 0, *map(_ptr, sums))
        self._launch(device, self._lib.aesmc_affine_backward_collect,
                     (_DTYPE_TAG[dtype], _ptr(ws), records, dx, dy, ctypes.byref(outs), self._stream(ws)),
                     lambda: records * 1024 * (8 if dtype == torch.float64 else 4), (ws, outs) + sums)
        return self._affine_grad_slots(None, None, sums, need, (None, None, None), scales)


    def affine_step_backward_unfused(self, x_prev, x, y_rows, transition, emission, proposal, scales, need, lw, lse,
                                     grad_lse=None, grad_x=None, grad_lw=None):
        """The same gradients by the launches K14 replaces — K12 (with x's gradient), the accumulation, K11 for
        the draw — the route for shapes K14 declines and its cross-check."""
        (Q, off_q) = proposal
        inner = list(need)
        inner[1] = True
        if grad_lse is None and grad_lw is None:      # only later steps' gradient arrives
            grad_lw = torch.zeros(x.shape[:2], dtype=x.dtype, device=x.device)
        grads = self.affine_logweight_backward(x_prev, x, y_rows, transition, emission, proposal, scales, inner,
                                               grad_lw=grad_lw, lw=lw, lse=lse, grad_lse=grad_lse)
        total = grads[1] if grad_x is None else grads[1] + grad_x
        grads[1] = None
        want_off = bool(need[8]) and off_q is not None
        gsrc, gw, rows = self.particle_affine_backward(total.contiguous(), x_prev, Q, bool(need[0]), bool(need[7]),
                                                       want_off)
        add = lambda a, b: b if a is None else a + b
        if need[0]:
            grads[0] = add(grads[0], gsrc)
        if need[7]:
            grads[7] = add(grads[7], gw)
        if want_off:
            grads[8] = add(grads[8], rows if off_q.dim() == 2 else rows.sum(dim=0))
        if need[11]:
            eps = (x - self.particle_affine(x_prev, Q, off_q)) / scales[2]
            grads[11] = add(grads[11], (total * eps).sum().reshape(scales[2].shape))
        return grads

    # ---- K7 ------------------------------------------------------------------------------------
    def particle_summary(self, log_w, value=None, want_log_ess=False, want_mean=False, want_second=False):
        """(log_ess [B], mean [B,...], second moment [B,...]) under w = softmax(log_w, dim=1); entries
        not asked for are None.  value [B,K,...] of log_w's dtype, may be strided."""
        tag = self._rows_operand(log_w, "log_weight")
        B, K = log_w.shape
        if K == 0:
            raise ValueError("aesmc_amd: particle summaries need at least one particle")
        log_w = log_w.contiguous()
        view, D, tail = None, 0, ()
        if want_mean or want_second:
            _require_hip(value, "value")
            if value.dtype != log_w.dtype or value.device != log_w.device:
                raise ValueError("aesmc_amd: value must be {} on {}".format(log_w.dtype, log_w.device))
            assert value.size()[:2] == log_w.size()
            tail = tuple(value.shape[2:])
            value, sv, D = self._view3(value)
            view = _lib.View3(_ptr(value), *sv)
        make = lambda shape: torch.empty(shape, dtype=log_w.dtype, device=log_w.device)
        log_ess = make((B,)) if want_log_ess else None
        mean = make((B,) + tail) if want_mean else None
        second = make((B,) + tail) if want_second else None
        if B == 0:
            return log_ess, mean, second
        if view is None or D == 0:
            view, D = None, 0
            if mean is not None:
                mean.zero_()        # rows without values: empty sums
            if second is not None:
                second.zero_()
        ws_bytes = int(self._lib.aesmc_particle_summary_workspace_bytes(tag, B, K, D))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=log_w.device) if ws_bytes else None
        self._launch(log_w.device, self._lib.aesmc_particle_summary,
                     (tag, _ptr(log_w), ctypes.byref(view) if view is not None else None,
                      _ptr(log_ess), _ptr(mean) if D > 0 else 0, _ptr(second) if D > 0 else 0, B, K, D,
                      _ptr(ws), ws_bytes, self._stream(log_w)),
                     lambda: log_w.numel() * log_w.element_size() + (self._unique_bytes(value) if view is not None else 0),
                     (log_w, value, view, log_ess, mean, second, ws))
        return log_ess, mean, second

    # ---- K21 -----------------------------------------------------------------------------------
    BACKWARD_SAMPLE_MAX_DIM = 256

    @staticmethod
    def backward_sample_covers(log_w, loc, target, scale, u, payload=None):
        """Whether `backward_sample` takes these operands: float32 / float64 throughout and all on one device, at least one
        particle, a transition term of at most 256 values per particle whose scale is one value or one per value."""
        if not (torch.is_tensor(log_w) and log_w.dim() == 2 and log_w.dtype in _DTYPE_TAG and log_w.size(1) > 0):
            return False
        if not (torch.is_tensor(u) and u.dim() == 2 and u.dtype == torch.float64 and u.size(0) == log_w.size(0) and
                u.device == log_w.device):
            return False
        if payload is not None and not (torch.is_tensor(payload) and payload.dim() >= 2 and payload.dtype == log_w.dtype and
                                        payload.device == log_w.device and
                                        tuple(payload.shape[:2]) == tuple(log_w.shape)):
            return False
        if loc is None:
            return target is None and scale is None
        if not all(torch.is_tensor(t) and t.dtype == log_w.dtype and t.device == log_w.device
                   for t in (loc, target, scale)):
            return False
        if loc.dim() < 2 or tuple(loc.shape[:2]) != tuple(log_w.shape) or target.dim() != loc.dim() or \
                tuple(target.shape[:2]) != tuple(u.shape) or tuple(target.shape[2:]) != tuple(loc.shape[2:]):
            return False
        D = 1
        for size in loc.shape[2:]:
            D *= size
        return 0 < D <= HipKernels.BACKWARD_SAMPLE_MAX_DIM and scale.dim() <= 1 and scale.numel() in (1, D)

    def backward_sample(self, log_w, loc, target, scale, u, payload=None):
        """One backward-simulation step (aesmc_backward_sample, K21): log_w [B,K], loc [B,K,*] (the transition's location
        per stored particle), target [B,M,*] (the trajectories' next states), scale one value or one per location value, u
        float64 [B,M]; loc = target = scale = None: no transition term (the last timestep).  Returns (idx int64 [B,M],
        payload[b, idx[b,m]] as [B,M,*] or None).  Views are taken as they are (element strides)."""
        tag = self._rows_operand(log_w, "log_weight")
        _require_hip(u, "uniforms")
        B, K = log_w.shape
        if u.dim() != 2 or u.size(0) != B or u.dtype != torch.float64 or u.device != log_w.device:
            raise ValueError("aesmc_amd: uniforms must be [{}, num_trajectories] float64 on {}".format(B, log_w.device))
        if not self.backward_sample_covers(log_w, loc, target, scale, u, payload):
            raise ValueError("aesmc_amd: backward_sample does not take these operands (see backward_sample_covers)")
        M = u.size(1)
        log_w, u = log_w.contiguous(), u.contiguous()
        views, keep, D, scale_stride = [None, None, None], [], 0, 0
        if loc is not None:
            for t in (loc, target, scale):
                _require_hip(t, "transition term")
            (loc, sl, D), (target, st, _) = self._view3(loc), self._view3(target)
            scale = scale.reshape(-1).contiguous()
            scale_stride = 0 if scale.numel() == 1 else 1
            views[0], views[1] = _lib.View3(_ptr(loc), *sl), _lib.View3(_ptr(target), *st)
            keep += [loc, target, scale]
        P, moved = 0, None
        if payload is not None:
            _require_hip(payload, "payload")
            tail = tuple(payload.shape[2:])
            payload, sp, P = self._view3(payload)
            moved = torch.empty((B, M) + tail, dtype=payload.dtype, device=payload.device)
            if P > 0:
                views[2] = _lib.View3(_ptr(payload), *sp)
            keep.append(payload)
        idx = torch.empty((B, M), dtype=torch.int64, device=log_w.device)
        if idx.numel() == 0:
            return idx, moved
        esz = log_w.element_size()
        refs = [ctypes.byref(v) if v is not None else None for v in views]
        self._launch(log_w.device, self._lib.aesmc_backward_sample,
                     (tag, _ptr(log_w), refs[0], refs[1], _ptr(scale) if D else 0, scale_stride, _ptr(u), _ptr(idx), refs[2],
                      _ptr(moved) if P else 0, _ptr(self.flags(log_w.device)), B, K, M, D, P, self._stream(log_w)),
                     lambda: B * K * esz * (1 + D) + B * M * (16 + esz * (D + 2 * P)),
                     tuple(keep) + (log_w, u, idx, moved) + tuple(views))
        return idx, moved

    # ---- K26 -----------------------------------------------------------------------------------
    CONDITIONAL_MAX_PARTICLES = 8192

    @staticmethod
    def conditional_ancestor_index_covers(log_w, u, loc=None, target=None, scale=None):
        """Whether `conditional_ancestor_index` takes these operands: float32 / float64 throughout and all on one device,
        1 to 8192 particles, one float64 uniform per slot, and either no transition term or loc [B,K,*], target [B,*] with
        the same trailing dims of at most 256 values and a scale of one value or one per value."""
        if not (torch.is_tensor(log_w) and log_w.dim() == 2 and log_w.dtype in _DTYPE_TAG and
                0 < log_w.size(1) <= HipKernels.CONDITIONAL_MAX_PARTICLES):
            return False
        if not (torch.is_tensor(u) and u.dtype == torch.float64 and tuple(u.shape) == tuple(log_w.shape) and
                u.device == log_w.device):
            return False
        if loc is None:
            return target is None and scale is None
        if not all(torch.is_tensor(t) and t.dtype == log_w.dtype and t.device == log_w.device
                   for t in (loc, target, scale)):
            return False
        if loc.dim() < 2 or tuple(loc.shape[:2]) != tuple(log_w.shape) or target.dim() != loc.dim() - 1 or \
                target.size(0) != log_w.size(0) or tuple(target.shape[1:]) != tuple(loc.shape[2:]):
            return False
        D = 1
        for size in loc.shape[2:]:
            D *= size
        return 0 < D <= HipKernels.BACKWARD_SAMPLE_MAX_DIM and scale.dim() <= 1 and scale.numel() in (1, D)

    def conditional_ancestor_index(self, log_w, u, loc=None, target=None, scale=None):
        """The ancestors of one conditional-SMC step (aesmc_conditional_ancestor_index, K26): log_w [B,K], u float64
        [B,K]; slots 0 .. K-2 draw multinomial ancestors from the weights, slot K-1 is pinned: it keeps ancestor K-1 (loc =
        target = scale = None), or draws it as K21 draws one trajectory whose next state is target [B,*], with loc [B,K,*]
        the transition's location per particle and scale one value or one per location value (ancestor sampling).
        Returns idx int64 [B,K].  Views are taken as they are (element strides)."""
        tag = self._rows_operand(log_w, "log_weight")
        _require_hip(u, "uniforms")
        B, K = log_w.shape
        if tuple(u.shape) != (B, K) or u.dtype != torch.float64 or u.device != log_w.device:
            raise ValueError("aesmc_amd: uniforms must be [{}, {}] float64 on {}".format(B, K, log_w.device))
        if not self.conditional_ancestor_index_covers(log_w, u, loc, target, scale):
            raise ValueError("aesmc_amd: conditional_ancestor_index does not take these operands (see "
                             "conditional_ancestor_index_covers)")
        log_w, u = log_w.contiguous(), u.contiguous()
        views, keep, D, scale_stride = [None, None], [], 0, 0
        if loc is not None:
            for t in (loc, target, scale):
                _require_hip(t, "transition term")
            (loc, sl, D), (target, st, _) = self._view3(loc), self._view3(target.unsqueeze(1))
            scale = scale.reshape(-1).contiguous()
            scale_stride = 0 if scale.numel() == 1 else 1
            views[0], views[1] = _lib.View3(_ptr(loc), *sl), _lib.View3(_ptr(target), *st)
            keep += [loc, target, scale]
        idx = torch.empty((B, K), dtype=torch.int64, device=log_w.device)
        if idx.numel() == 0:
            return idx
        esz = log_w.element_size()
        refs = [ctypes.byref(v) if v is not None else None for v in views]
        self._launch(log_w.device, self._lib.aesmc_conditional_ancestor_index,
                     (tag, _ptr(log_w), _ptr(u), refs[0], refs[1], _ptr(scale) if D else 0, scale_stride, _ptr(idx),
                      _ptr(self.flags(log_w.device)), B, K, D, self._stream(log_w)),
                     lambda: B * K * (esz * (1 + D) + 16) + B * D * esz,
                     tuple(keep) + (log_w, u, idx) + tuple(views))
        return idx

    # ---- K27 / K28 -----------------------------------------------------------------------------
    ADAPTED_MAX_DIM = 16

    @staticmethod
    def adapted_covers(loc, latent_dim, observation_dim):
        """Whether `affine_quadratic_logweight` / `adapted_draw` take a location like this: a float32 / float64 tensor
        [B,K,D] on the HIP device with D = latent_dim, both extents in 1 .. 16, and B K D within 32-bit element
        arithmetic."""
        if not (torch.is_tensor(loc) and loc.is_cuda and loc.dtype in _DTYPE_TAG and loc.dim() == 3):
            return False
        limit = HipKernels.ADAPTED_MAX_DIM
        return loc.size(2) == latent_dim and 1 <= latent_dim <= limit and 1 <= observation_dim <= limit and \
            loc.size(0) * loc.size(1) <= 0x7fffffff // limit

    def _adapted_operands(self, loc, what, **matrices):
        """The dtype tag of a [B,K,D] location and its float64 companions checked: name -> (tensor, shape)."""
        _require_hip(loc, what)
        tag = _tag(loc, what)
        if loc.dim() != 3:
            raise ValueError("aesmc_amd: {} must be [batch_size, num_particles, dim], got {}".format(what, tuple(loc.shape)))
        for name, (tensor, shape) in matrices.items():
            _require_hip(tensor, name)
            if tuple(tensor.shape) != tuple(shape) or tensor.dtype != torch.float64 or tensor.device != loc.device:
                raise ValueError("aesmc_amd: {} must be {} float64 on {}, got {} {} on {}".format(
                    name, tuple(shape), loc.device, tuple(tensor.shape), tensor.dtype, tensor.device))
        return tag

    def affine_quadratic_logweight(self, loc, P, offset, base):
        """The first-stage log-weights of an adapted step (aesmc_affine_quadratic_logweight, K27): loc [B,K,D] (a view is
        taken as it is), P float64 [Dy,D], offset float64 [B,Dy], base a Python float.  Returns [B,K] in loc's dtype:
        base - 1/2 |P loc + offset|^2, evaluated in float64."""
        B, K, D = loc.shape if torch.is_tensor(loc) and loc.dim() == 3 else (0, 0, 0)
        Dy = P.size(0) if torch.is_tensor(P) and P.dim() == 2 else 0
        tag = self._adapted_operands(loc, "location", P=(P, (Dy, D)), offset=(offset, (B, Dy)))
        if not self.adapted_covers(loc, D, Dy):
            raise ValueError("aesmc_amd: affine_quadratic_logweight does not take these operands (see adapted_covers)")
        P, offset = P.contiguous(), offset.contiguous()
        out = torch.empty((B, K), dtype=loc.dtype, device=loc.device)
        if out.numel() == 0:
            return out
        view = _lib.View3(_ptr(loc), *loc.stride())
        esz = loc.element_size()
        self._launch(loc.device, self._lib.aesmc_affine_quadratic_logweight,
                     (tag, ctypes.byref(view), _ptr(P), _ptr(offset), float(base), _ptr(out), B, K, D, Dy,
                      self._stream(loc)),
                     lambda: self._unique_bytes(loc) + B * K * esz + 8 * (Dy * D + B * Dy), (loc, P, offset, out, view))
        return out

    def adapted_draw(self, loc, index, M, offset, L, eps):
        """The draw of an adapted step (aesmc_adapted_draw, K28): loc [B,K,D] the transition's location of the STORED
        particles (a view is taken as it is), index int64 [B,K] or None (the identity), M and L float64 [D,D], offset
        float64 [B,D], eps [B,K,D] standard-normal noise in loc's dtype.  Returns x [B,K,D]: offset + M loc[index] +
        L eps, evaluated in float64.  An index outside [0, K) gives NaN there and FLAG_INDEX_OUT_OF_RANGE."""
        B, K, D = loc.shape if torch.is_tensor(loc) and loc.dim() == 3 else (0, 0, 0)
        tag = self._adapted_operands(loc, "location", M=(M, (D, D)), L=(L, (D, D)), offset=(offset, (B, D)))
        _require_hip(eps, "noise")
        self._expect(eps, loc.shape, loc, "noise")
        if not self.adapted_covers(loc, D, D):
            raise ValueError("aesmc_amd: adapted_draw does not take these operands (see adapted_covers)")
        if index is not None:
            index = as_index(index)
            if tuple(index.shape) != (B, K) or index.dtype != torch.int64 or index.device != loc.device:
                raise ValueError("aesmc_amd: index must be [{}, {}] int64 on {}".format(B, K, loc.device))
            index = index.contiguous()
        M, L, offset, eps = M.contiguous(), L.contiguous(), offset.contiguous(), eps.contiguous()
        if eps.data_ptr() % 16:      # (a slice of a larger block: the kernel stages the noise in 16-byte vectors)
            eps = eps.clone()
        out = torch.empty((B, K, D), dtype=loc.dtype, device=loc.device)
        if out.numel() == 0:
            return out
        view = _lib.View3(_ptr(loc), *loc.stride())
        esz = loc.element_size()
        self._launch(loc.device, self._lib.aesmc_adapted_draw,
                     (tag, ctypes.byref(view), _ptr(index), _ptr(M), _ptr(offset), _ptr(L), _ptr(eps), _ptr(out),
                      _ptr(self.flags(loc.device)), B, K, D, self._stream(loc)),
                     lambda: self._unique_bytes(loc) + B * K * (2 * D * esz + (8 if index is not None else 0)) +
                     8 * (2 * D * D + B * D), (loc, index, M, offset, L, eps, out, view))
        return out

    # ---- K29 / K30 -----------------------------------------------------------------------------
    def _adapted_workspace(self, device, B, K, D, Dy):
        """The float64 partial sums of a K29 / K30 launch (aesmc_adapted_backward_workspace_bytes): allocated per call from
        torch's caching allocator, which keeps the block per device like the other backward workspaces."""
        ws_bytes = int(self._lib.aesmc_adapted_backward_workspace_bytes(B, K, D, Dy))
        return torch.empty(ws_bytes, dtype=torch.uint8, device=device), ws_bytes

    def affine_quadratic_logweight_backward(self, loc, P, offset, grad, need_loc=True, need_P=True, need_offset=True):
        """The adjoint of `affine_quadratic_logweight` (aesmc_affine_quadratic_logweight_backward, K29) for the gradient
        grad [B,K] (loc's dtype) arriving at its output: (grad_loc [B,K,D] in loc's dtype, dense; grad_P float64 [Dy,D];
        grad_offset float64 [B,Dy]), None where `need_*` is false.  The gradient of `base` is grad.sum(): the caller's."""
        B, K, D = loc.shape if torch.is_tensor(loc) and loc.dim() == 3 else (0, 0, 0)
        Dy = P.size(0) if torch.is_tensor(P) and P.dim() == 2 else 0
        tag = self._adapted_operands(loc, "location", P=(P, (Dy, D)), offset=(offset, (B, Dy)))
        _require_hip(grad, "gradient")
        self._expect(grad, loc.shape[:2], loc, "gradient")
        if not self.adapted_covers(loc, D, Dy):
            raise ValueError("aesmc_amd: affine_quadratic_logweight_backward does not take these operands (see "
                             "adapted_covers)")
        P, offset, grad = P.contiguous(), offset.contiguous(), grad.contiguous()
        f64 = lambda shape, wanted: torch.empty(shape, dtype=torch.float64, device=loc.device) if wanted else None
        grad_loc = torch.empty((B, K, D), dtype=loc.dtype, device=loc.device) if need_loc else None
        grad_P, grad_offset = f64((Dy, D), need_P), f64((B, Dy), need_offset)
        if B * K == 0 or not (need_loc or need_P or need_offset):
            return (grad_loc,) + tuple(None if t is None else t.zero_() for t in (grad_P, grad_offset))
        ws, ws_bytes = self._adapted_workspace(loc.device, B, K, D, Dy) if (need_P or need_offset) else (None, 0)
        view = _lib.View3(_ptr(loc), *loc.stride())
        esz = loc.element_size()
        self._launch(loc.device, self._lib.aesmc_affine_quadratic_logweight_backward,
                     (tag, ctypes.byref(view), _ptr(P), _ptr(offset), _ptr(grad), _ptr(grad_loc), _ptr(grad_P),
                      _ptr(grad_offset), _ptr(ws), ws_bytes, B, K, D, Dy, self._stream(loc)),
                     lambda: self._unique_bytes(loc) + B * K * esz * (1 + (D if need_loc else 0)) +
                     8 * (2 * Dy * D + 2 * B * Dy), (loc, P, offset, grad, grad_loc, grad_P, grad_offset, ws, view))
        return grad_loc, grad_P, grad_offset

    def adapted_draw_backward(self, loc, index, M, L, eps, grad, need_h=True, need_M=True, need_L=True, need_r=True):
        """The adjoint of `adapted_draw` (aesmc_adapted_draw_backward, K30) for the gradient grad [B,K,D] arriving at its
        output: (h [B,K,D] in loc's dtype — the gradient of the GATHERED rows loc[b, index[b,k]]: `gather_backward` makes
        the location's of it —, grad_M float64 [D,D], grad_L float64 [D,D] (exactly zero above the diagonal), grad_r
        float64 [B,D]: the gradient of `offset`), None where `need_*` is false.  L is taken for its shape only.  An index
        outside [0, K) contributes nothing, gives a NaN row of h and FLAG_INDEX_OUT_OF_RANGE."""
        B, K, D = loc.shape if torch.is_tensor(loc) and loc.dim() == 3 else (0, 0, 0)
        tag = self._adapted_operands(loc, "location", M=(M, (D, D)), L=(L, (D, D)))
        for name, t in (("noise", eps), ("gradient", grad)):
            _require_hip(t, name)
            self._expect(t, loc.shape, loc, name)
        if not self.adapted_covers(loc, D, D):
            raise ValueError("aesmc_amd: adapted_draw_backward does not take these operands (see adapted_covers)")
        if index is not None:
            index = as_index(index)
            if tuple(index.shape) != (B, K) or index.dtype != torch.int64 or index.device != loc.device:
                raise ValueError("aesmc_amd: index must be [{}, {}] int64 on {}".format(B, K, loc.device))
            index = index.contiguous()
        M, eps, grad = M.contiguous(), eps.contiguous(), grad.contiguous()
        if eps.data_ptr() % 16:      # (slices of larger blocks: the kernel reads both in 16-byte vectors)
            eps = eps.clone()
        if grad.data_ptr() % 16:
            grad = grad.clone()
        f64 = lambda shape, wanted: torch.empty(shape, dtype=torch.float64, device=loc.device) if wanted else None
        h = torch.empty((B, K, D), dtype=loc.dtype, device=loc.device) if need_h else None
        grad_M, grad_L, grad_r = f64((D, D), need_M), f64((D, D), need_L), f64((B, D), need_r)
        if B * K == 0 or not (need_h or need_M or need_L or need_r):
            return (h,) + tuple(None if t is None else t.zero_() for t in (grad_M, grad_L, grad_r))
        reduces = need_M or need_L or need_r
        ws, ws_bytes = self._adapted_workspace(loc.device, B, K, D, D) if reduces else (None, 0)
        view = _lib.View3(_ptr(loc), *loc.stride())
        esz = loc.element_size()
        self._launch(loc.device, self._lib.aesmc_adapted_draw_backward,
                     (tag, ctypes.byref(view), _ptr(index), _ptr(M), _ptr(eps), _ptr(grad), _ptr(h), _ptr(grad_M),
                      _ptr(grad_L), _ptr(grad_r), _ptr(self.flags(loc.device)), _ptr(ws), ws_bytes, B, K, D,
                      self._stream(loc)),
                     lambda: (self._unique_bytes(loc) if need_M else 0) +
                     B * K * (D * esz * (1 + (1 if need_L else 0) + (1 if need_h else 0)) +
                              (8 if index is not None else 0)) + 8 * (3 * D * D + B * D),
                     (loc, index, M, eps, grad, h, grad_M, grad_L, grad_r, ws, view))
        return h, grad_M, grad_L, grad_r

    # ---- K31 -----------------------------------------------------------------------------------
    SWITCHING_MODEL_KEYS = ("cdf0", "cdf", "m0", "s0", "A", "b", "q", "C", "d", "r")

    def switching_limits(self):
        """(largest D, largest Dy, largest M) of `switching_kalman_step`, as the library exports them."""
        return (int(self._lib.aesmc_switching_max_latent_dim()), int(self._lib.aesmc_switching_max_observation_dim()),
                int(self._lib.aesmc_switching_max_regimes()))

    def switching_covers(self, observation, num_regimes, latent_dim, observation_dim, num_particles):
        """Whether `switching_kalman_step` takes a step like this: a float32 / float64 observation [B,Dy] on the HIP device
        with Dy = observation_dim, 1 <= D <= 8, 1 <= Dy <= 8, 1 <= M <= 16, and B K D(D+1)/2 within 32-bit element
        arithmetic."""
        if not (torch.is_tensor(observation) and observation.is_cuda and observation.dtype in _DTYPE_TAG and
                observation.dim() == 2 and observation.size(1) == observation_dim):
            return False
        max_d, max_dy, max_m = self.switching_limits()
        return 1 <= latent_dim <= max_d and 1 <= observation_dim <= max_dy and 1 <= num_regimes <= max_m and \
            observation.size(0) * num_particles <= 0x7fffffff // (max_d * (max_d + 1) // 2)

    def _switching_block(self, model, device):
        """(block, M, D, Dy) of a switching model: every tensor of SWITCHING_MODEL_KEYS validated (dense float64 of its
        shape on `device`), and the C structure that points at them."""
        A, C = model["A"], model["C"]
        M, D, Dy = (A.size(0), A.size(2), C.size(1)) if torch.is_tensor(A) and A.dim() == 3 and torch.is_tensor(C) and \
            C.dim() == 3 else (0, 0, 0)
        shapes = {"cdf0": (M,), "cdf": (M, M), "m0": (D,), "s0": (D,), "A": (M, D, D), "b": (M, D), "q": (M, D),
                  "C": (M, Dy, D), "d": (M, Dy), "r": (M, Dy)}
        for name in self.SWITCHING_MODEL_KEYS:
            tensor = model[name]
            _require_hip(tensor, name)
            if tuple(tensor.shape) != shapes[name] or tensor.dtype != torch.float64 or tensor.device != device or \
                    not tensor.is_contiguous():
                raise ValueError("aesmc_amd: {} must be dense {} float64 on {}, got {} {} on {}".format(
                    name, shapes[name], device, tuple(tensor.shape), tensor.dtype, tensor.device))
        return _lib.SwitchingModel(*([_ptr(model[name]) for name in self.SWITCHING_MODEL_KEYS] + [M, D, Dy])), M, D, Dy

    @staticmethod
    def _switching_state(state, B, K, D, device):
        """The stored (regime, mean, cov) of a step, validated and dense."""
        regime, mean, cov = state
        TD = D * (D + 1) // 2
        for tensor, shape, dtype, what in ((regime, (B, K), torch.int32, "regime"), (mean, (B, K, D), torch.float64, "mean"),
                                           (cov, (B, K, TD), torch.float64, "cov")):
            _require_hip(tensor, what)
            if tuple(tensor.shape) != shape or tensor.dtype != dtype or tensor.device != device:
                raise ValueError("aesmc_amd: {} must be {} {} on {}".format(what, shape, dtype, device))
        return regime.contiguous(), mean.contiguous(), cov.contiguous()

    @staticmethod
    def _switching_observed(observed, B, Dy, device):
        """The mask of a masked step (K39, K40, K41), validated and dense: torch.bool [B,Dy] on the observation's device,
        whose storage the entries read as uint8."""
        if not torch.is_tensor(observed) or observed.dtype != torch.bool or tuple(observed.shape) != (B, Dy) or \
                observed.device != device:
            raise ValueError("aesmc_amd: observed must be None or a [{}, {}] torch.bool tensor on {}, got {}".format(
                B, Dy, device, "{} {} on {}".format(tuple(observed.shape), observed.dtype, observed.device)
                if torch.is_tensor(observed) else type(observed).__name__))
        return observed.contiguous()

    @staticmethod
    def _switching_model_bytes(M, D, Dy, rows=True):
        """The algorithmic traffic of a switching model's operands: per regime A, b, q, C, d, r and, with `rows`, its row of the
        chain (a launch that draws from per-particle rows, or that draws nothing, does not read them)."""
        return 8 * M * ((M if rows else 0) + D * D + 2 * D + Dy * D + 2 * Dy)

    def _switching_kalman(self, name, entry, masked_name, model, state, index, uniforms, observation, observed, cdf=None,
                          pinned_regime=None, draw=False, pinned=False):
        """`switching_kalman_step`, `switching_kalman_draw` (`draw`: with `cdf`) and `switching_kalman_conditional_step`
        (`pinned`: with `pinned_regime`; both: `switching_kalman_conditional_draw`), called as `name`, which messages and the
        timer's entries carry.  Without `observed` the launch is the caller's own C `entry` (and so its unmasked kernel);
        with it, the masked entry, which takes both operands as nullable, recorded as `masked_name`."""
        _require_hip(observation, "observation")
        tag = _tag(observation, "observation")
        _require_hip(uniforms, "regime uniforms")
        device = observation.device
        if uniforms.dim() != 2 or uniforms.dtype != torch.float64 or uniforms.device != device:
            raise ValueError("aesmc_amd: regime uniforms must be [batch_size, num_particles] float64 on {}".format(device))
        B, K = uniforms.shape
        block, M, D, Dy = self._switching_block(model, device)
        TD = D * (D + 1) // 2
        if tuple(observation.shape) != (B, Dy):
            raise ValueError("aesmc_amd: observation must be [{}, {}], got {}".format(B, Dy, tuple(observation.shape)))
        if not self.switching_covers(observation, M, D, Dy, K):
            raise ValueError("aesmc_amd: {} does not take these operands (see switching_covers)".format(name))
        if draw:
            _require_hip(cdf, "cdf")
            if tuple(cdf.shape) != (B, K, M) or cdf.dtype != torch.float64 or cdf.device != device:
                raise ValueError("aesmc_amd: cdf must be {} float64 on {}".format((B, K, M), device))
            cdf = cdf.contiguous()
        if pinned:
            _require_hip(pinned_regime, "pinned_regime")
            if tuple(pinned_regime.shape) != (B,) or pinned_regime.dtype != torch.int32 or pinned_regime.device != device:
                raise ValueError("aesmc_amd: pinned_regime must be [{}] int32 on {}".format(B, device))
            pinned_regime = pinned_regime.contiguous()
        if state is not None:
            regime, mean, cov = self._switching_state(state, B, K, D, device)
            if index is not None:
                index = as_index(index)
                if tuple(index.shape) != (B, K) or index.dtype != torch.int64 or index.device != device:
                    raise ValueError("aesmc_amd: index must be [{}, {}] int64 on {}".format(B, K, device))
                index = index.contiguous()
        else:
            regime = mean = cov = index = None
        uniforms, observation = uniforms.contiguous(), observation.contiguous()
        if observed is not None:
            observed = self._switching_observed(observed, B, Dy, device)
        out_regime = torch.empty((B, K), dtype=torch.int32, device=device)
        out_mean = torch.empty((B, K, D), dtype=torch.float64, device=device)
        out_cov = torch.empty((B, K, TD), dtype=torch.float64, device=device)
        log_weight = torch.empty((B, K), dtype=torch.float64, device=device)
        outputs = (out_regime, out_mean, out_cov, log_weight)
        if log_weight.numel() == 0:
            return outputs
        # per particle: the uniform, the state written and (later steps) read, the weight, the index, the drawn-from row
        per_particle = 8 + (2 if state is not None else 1) * (4 + 8 * D + 8 * TD) + 8 + (8 if index is not None else 0) + \
            (8 * M if draw else 0)
        head = (tag, ctypes.byref(block), _ptr(regime), _ptr(mean), _ptr(cov), _ptr(index), _ptr(uniforms))
        tail = (_ptr(out_regime), _ptr(out_mean), _ptr(out_cov), _ptr(log_weight), _ptr(self.flags(device)), B, K,
                self._stream(observation))
        if observed is None:
            middle = ((_ptr(cdf),) if draw else ()) + ((_ptr(pinned_regime),) if pinned else ()) + (_ptr(observation),)
        else:
            entry, name = self._lib.aesmc_switching_kalman_masked_step, masked_name
            middle = (_ptr(cdf), _ptr(pinned_regime), _ptr(observation), _ptr(observed))
        self._launch(device, entry, head + middle + tail,
                     lambda: B * K * per_particle + (4 * B if pinned else 0) +
                     B * Dy * (observation.element_size() + (0 if observed is None else 1)) +
                     self._switching_model_bytes(M, D, Dy, rows=not draw),
                     (model, regime, mean, cov, index, uniforms, cdf, pinned_regime, observation, observed, out_regime, out_mean,
                      out_cov, log_weight, block), name=name)
        return outputs

    def switching_kalman_step(self, model, state, index, uniforms, observation, observed=None):
        """One step of the Rao-Blackwellised filter of a switching linear-Gaussian model (aesmc_switching_kalman_step, K31).
        model: a dict of dense float64 tensors cdf0 [M], cdf [M,M], m0 [D], s0 [D], A [M,D,D], b [M,D], q [M,D], C [M,Dy,D],
        d [M,Dy], r [M,Dy]; state: None (step 0) or (regime int32 [B,K], mean float64 [B,K,D], cov float64 [B,K,D(D+1)/2])
        — the STORED particles of the step before; index: int64 [B,K] or None (the identity); uniforms float64 [B,K];
        observation float32 / float64 [B,Dy].  Returns (regime, mean, cov, log_weight [B,K] float64), new tensors.  An index
        outside [0, K) or a stored regime outside [0, M) gives NaN there and FLAG_INDEX_OUT_OF_RANGE.
        observed: None, or torch.bool [B,Dy] — the masked entry (aesmc_switching_kalman_masked_step, K39): row b's step is the
        step of the model with the components deleted whose entry is False; y there is not used and may be NaN."""
        return self._switching_kalman("switching_kalman_step", self._lib.aesmc_switching_kalman_step,
                                      "switching_kalman_masked_step", model, state, index, uniforms, observation, observed)

    # ---- K32, K33 ------------------------------------------------------------------------------
    def _switching_lookahead(self, name, entry, masked_entry, scores, model, log_prior, state, observation, num_particles,
                             observed):
        """`switching_lookahead` and `switching_lookahead_scores` (`scores`), called as `name`: one validation, the caller's C
        `entry` (with `observed` its `masked_entry`), and the outputs in the order the entry takes them, which is the order
        returned: (log_weight, cdf), or (scores, log_weight)."""
        _require_hip(observation, "observation")
        tag = _tag(observation, "observation")
        device = observation.device
        block, M, D, Dy = self._switching_block(model, device)
        if observation.dim() != 2 or observation.size(1) != Dy:
            raise ValueError("aesmc_amd: observation must be [batch_size, {}], got {}".format(Dy, tuple(observation.shape)))
        B = observation.size(0)
        if state is None:
            if num_particles is None or int(num_particles) < 0:
                raise ValueError("aesmc_amd: {} without a state needs num_particles".format(name))
            K = int(num_particles)
        else:
            K = state[0].size(1) if torch.is_tensor(state[0]) and state[0].dim() == 2 else -1
            if num_particles is not None and int(num_particles) != K:
                raise ValueError("aesmc_amd: num_particles ({}) disagrees with the state ({})".format(num_particles, K))
        if not self.switching_covers(observation, M, D, Dy, K):
            raise ValueError("aesmc_amd: {} does not take these operands (see switching_covers)".format(name))
        _require_hip(log_prior, "log_prior")
        want = (M,) if state is None else (M, M)
        if tuple(log_prior.shape) != want or log_prior.dtype != torch.float64 or log_prior.device != device:
            raise ValueError("aesmc_amd: log_prior must be {} float64 on {}, got {} {} on {}".format(
                want, device, tuple(log_prior.shape), log_prior.dtype, log_prior.device))
        log_prior = log_prior.contiguous()
        regime, mean, cov = (None, None, None) if state is None else self._switching_state(state, B, K, D, device)
        observation = observation.contiguous()
        if observed is not None:
            observed = self._switching_observed(observed, B, Dy, device)
        log_weight = torch.empty((B, K), dtype=torch.float64, device=device)
        rows = torch.empty((B, K, M), dtype=torch.float64, device=device)      # the cumulative rows, or the scores
        outputs = (rows, log_weight) if scores else (log_weight, rows)
        if log_weight.numel() == 0:
            return outputs
        TD = D * (D + 1) // 2
        per_particle = (4 + 8 * D + 8 * TD if state is not None else 0) + 8 + 8 * M
        head = (tag, ctypes.byref(block), _ptr(log_prior), _ptr(regime), _ptr(mean), _ptr(cov), _ptr(observation))
        tail = (_ptr(outputs[0]), _ptr(outputs[1]), _ptr(self.flags(device)), B, K, self._stream(observation))
        self._launch(device, entry if observed is None else masked_entry,
                     head + tail if observed is None else head + (_ptr(observed),) + tail,
                     lambda: B * K * per_particle + B * Dy * (observation.element_size() + (0 if observed is None else 1)) +
                     self._switching_model_bytes(M, D, Dy),
                     (model, log_prior, regime, mean, cov, observation, observed, log_weight, rows, block))
        return outputs

    def switching_lookahead(self, model, log_prior, state, observation, num_particles=None, observed=None):
        """The look-ahead of the fully adapted filter of a switching linear-Gaussian model (aesmc_switching_lookahead, K32):
        per stored particle one Kalman prediction per regime, the exact first-stage log-weight log p(y | history) and the
        cumulative row of the exact regime posterior.  model, state, observation as `switching_kalman_step`'s; log_prior:
        float64 [M,M] with a state (log Pi), [M] without one (log pi0; `num_particles` then gives K).  Returns (log_weight
        [B,K], cdf [B,K,M]) float64, new tensors.  A stored regime outside [0, M) gives NaN there and
        FLAG_INDEX_OUT_OF_RANGE.  observed: as `switching_kalman_step`'s (aesmc_switching_masked_lookahead, K40)."""
        return self._switching_lookahead("switching_lookahead", self._lib.aesmc_switching_lookahead,
                                         self._lib.aesmc_switching_masked_lookahead, False, model, log_prior, state, observation,
                                         num_particles, observed)

    # ---- K43, K44 ------------------------------------------------------------------------------
    def switching_lookahead_scores(self, model, log_prior, state, observation, num_particles=None, observed=None):
        """`switching_lookahead` with the scores themselves in place of the cumulative row (aesmc_switching_lookahead_scores,
        K43; with `observed` aesmc_switching_masked_lookahead_scores): returns (scores [B,K,M], log_weight [B,K]) float64, new
        tensors — scores[b,k,j] = g_j as K32 defines it (-inf under a log-prior of -inf, NaN where a pivot is not positive
        under a finite one), log_weight K32's bit for bit.  Arguments, validation and flags as `switching_lookahead`'s."""
        return self._switching_lookahead("switching_lookahead_scores", self._lib.aesmc_switching_lookahead_scores,
                                         self._lib.aesmc_switching_masked_lookahead_scores, True, model, log_prior, state,
                                         observation, num_particles, observed)

    def switching_optimal_resample_max_candidates(self):
        """The most candidates K_in * M `switching_optimal_resample` keeps in LDS, as the library exports it."""
        return int(self._lib.aesmc_switching_optimal_resample_max_candidates())

    def switching_optimal_resample_covers(self, num_in, num_regimes, num_out, batch_size):
        """Whether `switching_optimal_resample` takes a step of K_in particles, M regimes and K_out slots in B rows."""
        return num_in >= 0 and num_out >= 0 and 1 <= num_regimes <= self.switching_limits()[2] and \
            num_in * num_regimes <= self.switching_optimal_resample_max_candidates() and batch_size * num_out <= 0x7fffffff

    def switching_optimal_resample(self, log_w, scores, u, num_slots):
        """Optimal resampling of a row's K_in * M candidates down to `num_slots` (aesmc_switching_optimal_resample, K44).
        log_w: float64 [B,K_in] or None (zeros); scores: float64 [B,K_in,M] (`switching_lookahead_scores`'); u: float64 [B] in
        [0, 1).  Returns (parent int64 [B,K_out], regime int32 [B,K_out], log_weight float64 [B,K_out] — normalised, -inf in
        dead slots —, lse float64 [B], count int32 [B]), new tensors.  A NaN candidate or a row without a finite maximum:
        every parent K_in, NaN weights and lse, count 0, and the flag.  K_in * M beyond
        `switching_optimal_resample_max_candidates` raises (ask `switching_optimal_resample_covers`)."""
        _require_hip(scores, "scores")
        _require_hip(u, "uniforms")
        device = scores.device
        if scores.dim() != 3 or scores.dtype != torch.float64:
            raise ValueError("aesmc_amd: scores must be [batch_size, num_particles, num_regimes] float64, got {} {}".format(
                tuple(scores.shape), scores.dtype))
        B, K_in, M = scores.shape
        K_out = int(num_slots)
        if K_out < 0:
            raise ValueError("aesmc_amd: num_slots must not be negative")
        if log_w is not None:
            _require_hip(log_w, "log_weight")
            if tuple(log_w.shape) != (B, K_in) or log_w.dtype != torch.float64 or log_w.device != device:
                raise ValueError("aesmc_amd: log_weight must be None or [{}, {}] float64 on {}".format(B, K_in, device))
            log_w = log_w.contiguous()
        if u.numel() != B or u.dtype != torch.float64 or u.device != device:
            raise ValueError("aesmc_amd: uniforms must be {} float64 values on {}".format(B, device))
        scores, u = scores.contiguous(), u.contiguous()
        parent = torch.empty((B, K_out), dtype=torch.int64, device=device)
        regime = torch.empty((B, K_out), dtype=torch.int32, device=device)
        log_weight = torch.empty((B, K_out), dtype=torch.float64, device=device)
        lse = torch.empty((B,), dtype=torch.float64, device=device)
        count = torch.empty((B,), dtype=torch.int32, device=device)
        if B == 0 or K_out == 0 or K_in == 0 or M == 0:
            return parent, regime, log_weight, lse.fill_(float("nan")), count.zero_()
        self._launch(device, self._lib.aesmc_switching_optimal_resample,
                     (_ptr(log_w), _ptr(scores), _ptr(u), _ptr(parent), _ptr(regime), _ptr(log_weight), _ptr(lse), _ptr(count),
                      _ptr(self.flags(device)), B, K_in, M, K_out, self._stream(scores)),
                     lambda: B * (K_in * (8 * M + (8 if log_w is not None else 0)) + 20 * K_out + 20),
                     (log_w, scores, u, parent, regime, log_weight, lse, count), name="switching_optimal_resample")
        return parent, regime, log_weight, lse, count

    def switching_kalman_draw(self, model, state, index, uniforms, cdf, observation, observed=None):
        """`switching_kalman_step` with the regime drawn from a cumulative row per particle (aesmc_switching_kalman_draw,
        K33): cdf float64 [B,K,M], read at the ancestor's position (`switching_lookahead`'s).  Returns (regime, mean, cov,
        log_likelihood [B,K] float64), new tensors; regimes, flags and NaNs as `switching_kalman_step`'s, and its
        `observed` (K39 with particle_cdf)."""
        return self._switching_kalman("switching_kalman_draw", self._lib.aesmc_switching_kalman_draw,
                                      "switching_kalman_masked_draw", model, state, index, uniforms, observation, observed,
                                      cdf=cdf, draw=True)

    # ---- K34, K35 ------------------------------------------------------------------------------
    def switching_backward_covers(self, observation, num_regimes, latent_dim, observation_dim, num_particles,
                                  num_trajectories):
        """Whether `switching_information_step` and `switching_backward_scores` take a backward step like this: what
        `switching_covers` asks of the observation and the model for B N trajectories and for B K particles, and B N K
        scores within 32-bit element arithmetic."""
        if not (self.switching_covers(observation, num_regimes, latent_dim, observation_dim, num_particles) and
                self.switching_covers(observation, num_regimes, latent_dim, observation_dim, num_trajectories)):
            return False
        return observation.size(0) * num_trajectories * max(num_particles, 1) <= 0x7fffffff

    def switching_information_step(self, model, regime_next, info, observation, observed=None):
        """The information step of Rao-Blackwellised backward simulation (aesmc_switching_information_step, K34).  model as
        `switching_kalman_step`'s; regime_next int32 [B,N]: the trajectories' regimes at time t+1; info: None (the zeros of
        the last step) or (omega float64 [B,N,D(D+1)/2], lam float64 [B,N,D], c float64 [B,N]) of time t+1; observation
        float32 / float64 [B,Dy]: that of time t+1.  Returns (omega, lam, c, factor [B,N,D(D+1)/2]) of time t, new tensors;
        factor is the packed lower factor of omega, a pivot at or below 2^-40 of the largest diagonal entry giving a zero
        column.  A regime outside [0, M) gives NaN there and FLAG_INDEX_OUT_OF_RANGE.  observed: as
        `switching_kalman_step`'s (aesmc_switching_masked_information_step, K41)."""
        _require_hip(observation, "observation")
        tag = _tag(observation, "observation")
        _require_hip(regime_next, "regime_next")
        device = observation.device
        if regime_next.dim() != 2 or regime_next.dtype != torch.int32 or regime_next.device != device:
            raise ValueError("aesmc_amd: regime_next must be [batch_size, num_trajectories] int32 on {}".format(device))
        B, N = regime_next.shape
        block, M, D, Dy = self._switching_block(model, device)
        TD = D * (D + 1) // 2
        if tuple(observation.shape) != (B, Dy):
            raise ValueError("aesmc_amd: observation must be [{}, {}], got {}".format(B, Dy, tuple(observation.shape)))
        if not self.switching_covers(observation, M, D, Dy, N):
            raise ValueError("aesmc_amd: switching_information_step does not take these operands (see "
                             "switching_backward_covers)")
        omega = lam = c = None
        if info is not None:
            omega, lam, c = info
            for tensor, shape, what in ((omega, (B, N, TD), "omega"), (lam, (B, N, D), "lam"), (c, (B, N), "c")):
                _require_hip(tensor, what)
                if tuple(tensor.shape) != shape or tensor.dtype != torch.float64 or tensor.device != device:
                    raise ValueError("aesmc_amd: {} must be {} float64 on {}".format(what, shape, device))
            omega, lam, c = omega.contiguous(), lam.contiguous(), c.contiguous()
        regime_next, observation = regime_next.contiguous(), observation.contiguous()
        if observed is not None:
            observed = self._switching_observed(observed, B, Dy, device)
        out_omega = torch.empty((B, N, TD), dtype=torch.float64, device=device)
        out_lam = torch.empty((B, N, D), dtype=torch.float64, device=device)
        out_c = torch.empty((B, N), dtype=torch.float64, device=device)
        factor = torch.empty((B, N, TD), dtype=torch.float64, device=device)
        if out_c.numel() == 0:
            return out_omega, out_lam, out_c, factor
        per_trajectory = 4 + (2 if info is not None else 1) * 8 * (TD + D + 1) + 8 * TD
        head = (tag, ctypes.byref(block), _ptr(regime_next), _ptr(omega), _ptr(lam), _ptr(c), _ptr(observation))
        tail = (_ptr(out_omega), _ptr(out_lam), _ptr(out_c), _ptr(factor), _ptr(self.flags(device)), B, N,
                self._stream(observation))
        self._launch(device, self._lib.aesmc_switching_information_step if observed is None else
                     self._lib.aesmc_switching_masked_information_step,
                     head + tail if observed is None else head + (_ptr(observed),) + tail,
                     lambda: B * N * per_trajectory + B * Dy * (observation.element_size() + (0 if observed is None else 1)) +
                     self._switching_model_bytes(M, D, Dy, rows=False),
                     (model, regime_next, omega, lam, c, observation, observed, out_omega, out_lam, out_c, factor, block))
        return out_omega, out_lam, out_c, factor

    def switching_backward_scores(self, log_Pi, regime_next, factor, lam, state, log_w=None):
        """The pair scores of Rao-Blackwellised backward simulation (aesmc_switching_backward_scores, K35): log_Pi float64
        [M,M] (-inf where a probability is 0); regime_next int32 [B,N]; factor [B,N,D(D+1)/2] and lam [B,N,D]:
        `switching_information_step`'s; state: the stored (regime int32 [B,K], mean [B,K,D], cov [B,K,D(D+1)/2]) of step t;
        log_w float64 [B,K] or None (equal weights).  Returns scores float64 [B,N,K], a new tensor: -inf where the
        transition is impossible, NaN and FLAG_INDEX_OUT_OF_RANGE for a regime outside [0, M) on either side."""
        _require_hip(log_Pi, "log_Pi")
        _require_hip(regime_next, "regime_next")
        device = log_Pi.device
        if log_Pi.dim() != 2 or log_Pi.size(0) != log_Pi.size(1) or log_Pi.dtype != torch.float64:
            raise ValueError("aesmc_amd: log_Pi must be [M, M] float64, got {} {}".format(tuple(log_Pi.shape), log_Pi.dtype))
        M = log_Pi.size(0)
        if regime_next.dim() != 2 or regime_next.dtype != torch.int32 or regime_next.device != device:
            raise ValueError("aesmc_amd: regime_next must be [batch_size, num_trajectories] int32 on {}".format(device))
        B, N = regime_next.shape
        D = lam.size(-1) if torch.is_tensor(lam) and lam.dim() == 3 else 0
        TD = D * (D + 1) // 2
        for tensor, shape, what in ((factor, (B, N, TD), "factor"), (lam, (B, N, D), "lam")):
            _require_hip(tensor, what)
            if tuple(tensor.shape) != shape or tensor.dtype != torch.float64 or tensor.device != device:
                raise ValueError("aesmc_amd: {} must be {} float64 on {}".format(what, shape, device))
        K = state[0].size(1) if torch.is_tensor(state[0]) and state[0].dim() == 2 else -1
        regime, mean, cov = self._switching_state(state, B, K, D, device)
        if log_w is not None:
            _require_hip(log_w, "log_weight")
            if tuple(log_w.shape) != (B, K) or log_w.dtype != torch.float64 or log_w.device != device:
                raise ValueError("aesmc_amd: log_weight must be {} float64 on {}".format((B, K), device))
            log_w = log_w.contiguous()
        max_d, _, max_m = self.switching_limits()
        limit = 0x7fffffff
        if not (1 <= D <= max_d and 1 <= M <= max_m and B * N * max(K, 1) <= limit and
                B * max(K, N) <= limit // (max_d * (max_d + 1) // 2)):
            raise ValueError("aesmc_amd: switching_backward_scores does not take these operands (see "
                             "switching_backward_covers)")
        log_Pi, regime_next, factor, lam = log_Pi.contiguous(), regime_next.contiguous(), factor.contiguous(), lam.contiguous()
        scores = torch.empty((B, N, K), dtype=torch.float64, device=device)
        if scores.numel() == 0:
            return scores
        self._launch(device, self._lib.aesmc_switching_backward_scores,
                     (_ptr(log_Pi), _ptr(regime_next), _ptr(factor), _ptr(lam), _ptr(regime), _ptr(mean), _ptr(cov),
                      _ptr(log_w), _ptr(scores), _ptr(self.flags(device)), B, K, N, M, D, self._stream(log_Pi)),
                     lambda: 8 * B * N * K + B * N * (4 + 8 * (TD + D)) * ((K + 255) // 256) +
                     B * K * (4 + 8 * (D + TD) + (8 if log_w is not None else 0)) * ((N + 15) // 16),
                     (log_Pi, regime_next, factor, lam, regime, mean, cov, log_w, scores),
                     name="switching_backward_scores")
        return scores

    # ---- K36 -----------------------------------------------------------------------------------
    def switching_smooth_combine(self, model, regime_next, filtered, factor, lam, omega_next=None, cov_next=None,
                                 observed_next=None):
        """The two-filter combination of the state smoother (aesmc_switching_smooth_combine, K36).  filtered: (mean float64
        [B,N,D], cov float64 [B,N,D(D+1)/2]), the conditional filter's of time t; factor [B,N,D(D+1)/2], lam [B,N,D]:
        `switching_information_step`'s of time t.  The lag-one cross-covariance is formed when cov_next (the smoothed packed
        covariance of time t+1) is given: model as `switching_kalman_step`'s, regime_next int32 [B,N] (the regimes at t+1),
        omega_next: `switching_information_step`'s omega of time t+1 or None (t+1 = T-1).  Without cov_next the model,
        regime_next and omega_next are not read (pass None).  Returns (mean [B,N,D], cov [B,N,D(D+1)/2], cross [B,N,D,D] or
        None), new tensors.  With cov_next a regime outside [0, M) gives NaN there and FLAG_INDEX_OUT_OF_RANGE.
        observed_next: None, or torch.bool [B,Dy], which components of y_{t+1} were observed — the masked entry
        (aesmc_switching_masked_smooth_combine, K42), with cov_next only: the cross-covariance alone depends on it."""
        mean, cov = filtered
        _require_hip(mean, "mean")
        device = mean.device
        if mean.dim() != 3 or mean.dtype != torch.float64:
            raise ValueError("aesmc_amd: mean must be [batch_size, num_trajectories, D] float64, got {} {}".format(
                tuple(mean.shape), mean.dtype))
        B, N, D = mean.shape
        TD = D * (D + 1) // 2
        cross = cov_next is not None
        wanted = [(cov, (B, N, TD), "cov"), (factor, (B, N, TD), "factor"), (lam, (B, N, D), "lam")]
        if cross:
            wanted.append((cov_next, (B, N, TD), "cov_next"))
            if omega_next is not None:
                wanted.append((omega_next, (B, N, TD), "omega_next"))
        elif model is not None or regime_next is not None or omega_next is not None:
            raise ValueError("aesmc_amd: switching_smooth_combine reads model, regime_next and omega_next only with cov_next")
        for tensor, shape, what in wanted:
            _require_hip(tensor, what)
            if tuple(tensor.shape) != shape or tensor.dtype != torch.float64 or tensor.device != device:
                raise ValueError("aesmc_amd: {} must be {} float64 on {}".format(what, shape, device))
        max_d, max_dy, max_m = self.switching_limits()
        block, M, Dy = None, 0, 0
        if cross:
            _require_hip(regime_next, "regime_next")
            if tuple(regime_next.shape) != (B, N) or regime_next.dtype != torch.int32 or regime_next.device != device:
                raise ValueError("aesmc_amd: regime_next must be [{}, {}] int32 on {}".format(B, N, device))
            block, M, model_d, Dy = self._switching_block(model, device)
            if model_d != D:
                raise ValueError("aesmc_amd: the model's latent has {} values, the mean {}".format(model_d, D))
            regime_next, cov_next = regime_next.contiguous(), cov_next.contiguous()
            omega_next = None if omega_next is None else omega_next.contiguous()
            if observed_next is not None:
                observed_next = self._switching_observed(observed_next, B, Dy, device)
        elif observed_next is not None:
            raise ValueError("aesmc_amd: switching_smooth_combine reads observed_next only with cov_next")
        if not (1 <= D <= max_d and M <= max_m and Dy <= max_dy and B * N <= 0x7fffffff // (max_d * max_d)):
            raise ValueError("aesmc_amd: switching_smooth_combine does not take these operands (see switching_covers)")
        mean, cov, factor, lam = mean.contiguous(), cov.contiguous(), factor.contiguous(), lam.contiguous()
        out_mean = torch.empty((B, N, D), dtype=torch.float64, device=device)
        out_cov = torch.empty((B, N, TD), dtype=torch.float64, device=device)
        out_cross = torch.empty((B, N, D, D), dtype=torch.float64, device=device) if cross else None
        if out_mean.numel() == 0:
            return out_mean, out_cov, out_cross
        per_trajectory = 8 * (2 * D + 3 * TD) + \
            ((4 + 8 * (TD + D * D) + (8 * TD if omega_next is not None else 0)) if cross else 0)
        head = (None if block is None else ctypes.byref(block), _ptr(regime_next), _ptr(mean), _ptr(cov), _ptr(factor),
                _ptr(lam), _ptr(omega_next), _ptr(cov_next))
        tail = (_ptr(out_mean), _ptr(out_cov), _ptr(out_cross), _ptr(self.flags(device)), B, N, D, self._stream(mean))
        self._launch(device, self._lib.aesmc_switching_smooth_combine if observed_next is None else
                     self._lib.aesmc_switching_masked_smooth_combine,
                     head + tail if observed_next is None else head + (_ptr(observed_next),) + tail,
                     lambda: B * N * per_trajectory + (0 if observed_next is None else B * Dy) +
                     self._switching_model_bytes(M, D, Dy, rows=False),
                     (model, regime_next, mean, cov, factor, lam, omega_next, cov_next, observed_next, out_mean, out_cov, out_cross,
                      block))
        return out_mean, out_cov, out_cross

    # ---- K47 -----------------------------------------------------------------------------------
    def switching_state_draw(self, model, regimes, means, covs, noise, following=None):
        """A draw of the continuous state along regime paths, the whole backward pass in one launch
        (aesmc_switching_state_draw, K47).  model as `switching_kalman_step`'s; regimes int32 [T,B,N]; means float64
        [T,B,N,D] and covs float64 [T,B,N,D(D+1)/2]: the conditional filter's, stacked; noise float64 [T,B,N,D]: standard
        normals; following: None, or (regime_next int32 [B,N], z_next float64 [B,N,D]) — the regime and the drawn state of
        time T, for a pass in chunks (with T = 1 exactly one conditioning step).  Returns states float64 [T,B,N,D], a new
        tensor.  A regime outside [0, M) where it is read (regimes[t], t >= 1, and regime_next) gives NaN at every earlier
        time of that trajectory and FLAG_INDEX_OUT_OF_RANGE."""
        _require_hip(means, "means")
        device = means.device
        if means.dim() != 4 or means.dtype != torch.float64 or means.size(0) < 1:
            raise ValueError("aesmc_amd: means must be [T, batch_size, num_trajectories, D] float64 with T >= 1, got {} {}"
                             .format(tuple(means.shape), means.dtype))
        T, B, N, D = means.shape
        TD = D * (D + 1) // 2
        for tensor, shape, what in ((covs, (T, B, N, TD), "covs"), (noise, (T, B, N, D), "noise")):
            _require_hip(tensor, what)
            if tuple(tensor.shape) != shape or tensor.dtype != torch.float64 or tensor.device != device:
                raise ValueError("aesmc_amd: {} must be {} float64 on {}".format(what, shape, device))
        _require_hip(regimes, "regimes")
        if tuple(regimes.shape) != (T, B, N) or regimes.dtype != torch.int32 or regimes.device != device:
            raise ValueError("aesmc_amd: regimes must be [{}, {}, {}] int32 on {}".format(T, B, N, device))
        block, M, model_d, Dy = self._switching_block(model, device)
        if model_d != D:
            raise ValueError("aesmc_amd: the model's latent has {} values, the means {}".format(model_d, D))
        regime_next = z_next = None
        if following is not None:
            regime_next, z_next = following
            _require_hip(regime_next, "regime_next")
            _require_hip(z_next, "z_next")
            if tuple(regime_next.shape) != (B, N) or regime_next.dtype != torch.int32 or regime_next.device != device:
                raise ValueError("aesmc_amd: regime_next must be [{}, {}] int32 on {}".format(B, N, device))
            if tuple(z_next.shape) != (B, N, D) or z_next.dtype != torch.float64 or z_next.device != device:
                raise ValueError("aesmc_amd: z_next must be {} float64 on {}".format((B, N, D), device))
            regime_next, z_next = regime_next.contiguous(), z_next.contiguous()
        max_d, max_dy, max_m = self.switching_limits()
        if not (1 <= D <= max_d and 1 <= M <= max_m and 1 <= Dy <= max_dy and B * N <= 0x7fffffff // (max_d * max_d)):
            raise ValueError("aesmc_amd: switching_state_draw does not take these operands (see switching_covers)")
        regimes, means, covs, noise = regimes.contiguous(), means.contiguous(), covs.contiguous(), noise.contiguous()
        states = torch.empty((T, B, N, D), dtype=torch.float64, device=device)
        if B * N == 0:
            return states
        self._launch(device, self._lib.aesmc_switching_state_draw,
                     (ctypes.byref(block), _ptr(regimes), _ptr(means), _ptr(covs), _ptr(noise), _ptr(regime_next),
                      _ptr(z_next), _ptr(states), _ptr(self.flags(device)), T, B, N, self._stream(means)),
                     lambda: B * N * (T * (8 * (3 * D + TD)) + 4 * (T - 1) + (4 + 8 * D if following is not None else 0)) +
                     self._switching_model_bytes(M, D, Dy, rows=False) - 8 * M * (Dy * D + 2 * Dy),
                     (model, regimes, means, covs, noise, regime_next, z_next, states, block))
        return states

    # ---- K50, K51 ------------------------------------------------------------------------------
    def switching_collapse(self, means, covs, log_weights):
        """The moment-matching collapse of Gaussian mixtures (aesmc_switching_collapse, K50): group (b,g) of N weighted
        components becomes one Gaussian.  log_weights float64 [B,G,N]; means float64 [B,G,N,D] and covs float64
        [B,G,N,D(D+1)/2] (packed) — or [B,N,D] and [B,N,D(D+1)/2]: the shared-components form, the row's N components under
        every one of its G weight rows.  Returns (log_mass [B,G], mean [B,G,D], cov [B,G,D(D+1)/2]) float64, new tensors.
        A group of weights all -inf: -inf, zeros, zeros; a component of weight -inf is not read; a NaN weight: NaN."""
        _require_hip(log_weights, "log_weights")
        device = log_weights.device
        if log_weights.dim() != 3 or log_weights.dtype != torch.float64:
            raise ValueError("aesmc_amd: log_weights must be [batch_size, groups, components] float64, got {} {}".format(
                tuple(log_weights.shape), log_weights.dtype))
        B, G, N = log_weights.shape
        _require_hip(means, "means")
        shared = means.dim() == 3
        lead = (B, N) if shared else (B, G, N)
        D = means.size(-1) if means.dim() in (3, 4) else 0
        TD = D * (D + 1) // 2
        for tensor, shape, what in ((means, lead + (D,), "means"), (covs, lead + (TD,), "covs")):
            _require_hip(tensor, what)
            if D < 1 or tuple(tensor.shape) != shape or tensor.dtype != torch.float64 or tensor.device != device:
                raise ValueError("aesmc_amd: {} must be {} (or without the groups: shared) float64 on {}, got {} {} on {}"
                                 .format(what, (B, G, N, D if what == "means" else TD), device, tuple(tensor.shape),
                                         tensor.dtype, tensor.device))
        if D > self.switching_limits()[0] or N > 256 or G > 256 or B * G > 0x7fffffff:
            raise ValueError("aesmc_amd: switching_collapse takes D <= 8 and at most 256 groups of at most 256 components")
        means, covs, log_weights = means.contiguous(), covs.contiguous(), log_weights.contiguous()
        log_mass = torch.empty((B, G), dtype=torch.float64, device=device)
        mean = torch.empty((B, G, D), dtype=torch.float64, device=device)
        cov = torch.empty((B, G, TD), dtype=torch.float64, device=device)
        if B * G == 0:
            return log_mass, mean, cov
        self._launch(device, self._lib.aesmc_switching_collapse,
                     (_ptr(means), 0 if shared else N * D, _ptr(covs), 0 if shared else N * TD, _ptr(log_weights),
                      _ptr(log_mass), _ptr(mean), _ptr(cov), B, G, N, D, self._stream(log_weights)),
                     lambda: 8 * (B * (1 if shared else G) * N * (D + TD) + B * G * (N + 1 + D + TD)),
                     (means, covs, log_weights, log_mass, mean, cov))
        return log_mass, mean, cov

    def switching_pair_smooth(self, model, mean, cov, mean_next, cov_next):
        """A Rauch-Tung-Striebel step between mixture components (aesmc_switching_pair_smooth, K51).  model as
        `switching_kalman_step`'s (A, b, q are read); mean float64 [B,M,D] and cov float64 [B,M,D(D+1)/2]: the components
        filtered at t; mean_next, cov_next: the same shapes, smoothed at t+1.  Returns (means [B,M,M,D], covs
        [B,M,M,D(D+1)/2]) float64, new tensors: entry (b,i,j) is component i smoothed against regime j's component."""
        _require_hip(mean, "mean")
        device = mean.device
        block, M, D, Dy = self._switching_block(model, device)
        TD = D * (D + 1) // 2
        B = mean.size(0) if mean.dim() == 3 else -1
        for tensor, shape, what in ((mean, (B, M, D), "mean"), (cov, (B, M, TD), "cov"), (mean_next, (B, M, D), "mean_next"),
                                    (cov_next, (B, M, TD), "cov_next")):
            _require_hip(tensor, what)
            if tuple(tensor.shape) != shape or tensor.dtype != torch.float64 or tensor.device != device:
                raise ValueError("aesmc_amd: {} must be {} float64 on {}".format(what, ("batch_size",) + shape[1:], device))
        max_d, max_dy, max_m = self.switching_limits()
        if not (1 <= D <= max_d and 1 <= M <= max_m and 1 <= Dy <= max_dy and B * M * M <= 0x7fffffff):
            raise ValueError("aesmc_amd: switching_pair_smooth does not take these operands (see switching_covers)")
        mean, cov, mean_next, cov_next = mean.contiguous(), cov.contiguous(), mean_next.contiguous(), cov_next.contiguous()
        means = torch.empty((B, M, M, D), dtype=torch.float64, device=device)
        covs = torch.empty((B, M, M, TD), dtype=torch.float64, device=device)
        if B == 0:
            return means, covs
        self._launch(device, self._lib.aesmc_switching_pair_smooth,
                     (ctypes.byref(block), _ptr(mean), _ptr(cov), _ptr(mean_next), _ptr(cov_next), _ptr(means), _ptr(covs), B,
                      self._stream(mean)),
                     lambda: 8 * B * M * (D + TD) * (2 + M) + self._switching_model_bytes(M, D, Dy, rows=False) -
                     8 * M * (Dy * D + 2 * Dy),
                     (model, mean, cov, mean_next, cov_next, means, covs, block))
        return means, covs

    # ---- K52, K53, K54 -------------------------------------------------------------------------
    SWITCHING_GRADIENTS = ("m0", "s0", "A", "b", "q", "C", "d", "r")

    def switching_kalman_step_backward(self, model, regime, state, observation, grad_mean, grad_cov, grad_log_weight,
                                       observed=None, need_state=True, need=SWITCHING_GRADIENTS):
        """The adjoint of `switching_kalman_step` with the regime given (aesmc_switching_kalman_step_backward, K52; with
        `observed` aesmc_switching_kalman_masked_step_backward, K53).  model, observation, observed as the step's; regime
        int32 [B,K]: what the step returned; state: None (step 0) or (mean [B,K,D], cov [B,K,D(D+1)/2]), what it was given;
        grad_mean [B,K,D], grad_cov [B,K,D(D+1)/2], grad_log_weight [B,K] float64: the gradients arriving at its outputs.
        Returns (grad_mean_in, grad_cov_in, grads): the per-slot two None at step 0 or without `need_state` (a bool for
        both, or a pair (mean, cov) for each alone); grads a dict
        of the names in `need` (of SWITCHING_GRADIENTS; m0 and s0 only at step 0, where A, b and q are zero) to new float64
        tensors of the operands' shapes.  Only what is asked for is computed; the per-regime sums go through a workspace
        of aesmc_switching_backward_workspace_bytes from torch's caching allocator, per call."""
        _require_hip(observation, "observation")
        tag = _tag(observation, "observation")
        device = observation.device
        block, M, D, Dy = self._switching_block(model, device)
        TD = D * (D + 1) // 2
        B = observation.size(0) if observation.dim() == 2 else -1
        K = regime.size(1) if torch.is_tensor(regime) and regime.dim() == 2 else -1
        if tuple(observation.shape) != (B, Dy):
            raise ValueError("aesmc_amd: observation must be [batch_size, {}], got {}".format(Dy, tuple(observation.shape)))
        if not self.switching_covers(observation, M, D, Dy, max(K, 0)):
            raise ValueError("aesmc_amd: switching_kalman_step_backward does not take these operands (see switching_covers)")
        later = state is not None
        mean = cov = None
        if later:
            regime, mean, cov = self._switching_state((regime,) + tuple(state), B, K, D, device)
        else:
            _require_hip(regime, "regime")
            if tuple(regime.shape) != (B, K) or regime.dtype != torch.int32 or regime.device != device:
                raise ValueError("aesmc_amd: regime must be {} int32 on {}".format((B, K), device))
            regime = regime.contiguous()
        arriving = []
        for tensor, shape, what in ((grad_mean, (B, K, D), "grad_mean"), (grad_cov, (B, K, TD), "grad_cov"),
                                    (grad_log_weight, (B, K), "grad_log_weight")):
            _require_hip(tensor, what)
            if tuple(tensor.shape) != shape or tensor.dtype != torch.float64 or tensor.device != device:
                raise ValueError("aesmc_amd: {} must be {} float64 on {}".format(what, shape, device))
            arriving.append(tensor.contiguous())
        observation = observation.contiguous()
        if observed is not None:
            observed = self._switching_observed(observed, B, Dy, device)
        need = tuple(name for name in self.SWITCHING_GRADIENTS if name in need and not (later and name in ("m0", "s0")))
        need_mean, need_cov = need_state if isinstance(need_state, (tuple, list)) else (need_state, need_state)
        need_mean, need_cov = bool(need_mean) and later, bool(need_cov) and later
        need_state = need_mean or need_cov
        if not need and not need_state:
            raise ValueError("aesmc_amd: switching_kalman_step_backward was asked for nothing")
        new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=device)
        grad_mean_in, grad_cov_in = new(B, K, D) if need_mean else None, new(B, K, TD) if need_cov else None
        grads = {name: new(*model[name].shape) for name in need}
        if B * K == 0:
            for value in grads.values():
                value.zero_()
            return grad_mean_in, grad_cov_in, grads
        ws_bytes = int(self._lib.aesmc_switching_backward_workspace_bytes(B, K, D, Dy)) if need else 0
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=device) if need else None
        head = (tag, ctypes.byref(block), _ptr(regime), _ptr(mean), _ptr(cov), _ptr(observation))
        tail = tuple(_ptr(t) for t in arriving) + (_ptr(grad_mean_in), _ptr(grad_cov_in)) + \
            tuple(_ptr(grads.get(name)) for name in self.SWITCHING_GRADIENTS) + \
            (_ptr(ws), ws_bytes, _ptr(self.flags(device)), B, K, self._stream(observation))
        entry, name, middle = (self._lib.aesmc_switching_kalman_step_backward, "switching_kalman_step_backward", ()) \
            if observed is None else (self._lib.aesmc_switching_kalman_masked_step_backward,
                                      "switching_kalman_masked_step_backward", (_ptr(observed),))
        self._launch(device, entry, head + middle + tail,
                     lambda: B * K * (4 + 8 * (D + TD + 1) + (8 * (D + TD) if later else 0) +
                                      (8 * D if need_mean else 0) + (8 * TD if need_cov else 0)) + 2 * ws_bytes +
                     B * Dy * (observation.element_size() + (0 if observed is None else 1)) +
                     self._switching_model_bytes(M, D, Dy, rows=False),
                     (model, regime, mean, cov, observation, observed, arriving, grad_mean_in, grad_cov_in, grads, ws, block),
                     name=name)
        return grad_mean_in, grad_cov_in, grads

    def switching_collapse_backward(self, means, covs, log_weights, grad_log_mass, grad_mean, grad_cov, need_means=True,
                                    need_covs=True, need_log_weights=True):
        """The adjoint of `switching_collapse` (aesmc_switching_collapse_backward, K54): its three operands and the float64
        gradients arriving at log_mass [B,G], mean [B,G,D] and cov [B,G,D(D+1)/2].  Returns (grad_means, grad_covs,
        grad_log_weights) in the operands' shapes — for shared components [B,N,.]: the sum over the row's groups in
        ascending order — None where not asked for."""
        _require_hip(log_weights, "log_weights")
        device = log_weights.device
        if log_weights.dim() != 3 or log_weights.dtype != torch.float64:
            raise ValueError("aesmc_amd: log_weights must be [batch_size, groups, components] float64, got {} {}".format(
                tuple(log_weights.shape), log_weights.dtype))
        B, G, N = log_weights.shape
        _require_hip(means, "means")
        shared = means.dim() == 3
        lead = (B, N) if shared else (B, G, N)
        D = means.size(-1) if means.dim() in (3, 4) else 0
        TD = D * (D + 1) // 2
        checked = []
        for tensor, shape, what in ((means, lead + (D,), "means"), (covs, lead + (TD,), "covs"),
                                    (grad_log_mass, (B, G), "grad_log_mass"), (grad_mean, (B, G, D), "grad_mean"),
                                    (grad_cov, (B, G, TD), "grad_cov")):
            _require_hip(tensor, what)
            if D < 1 or tuple(tensor.shape) != shape or tensor.dtype != torch.float64 or tensor.device != device:
                raise ValueError("aesmc_amd: {} must be {} float64 on {}, got {} {} on {}".format(
                    what, shape, device, tuple(tensor.shape), tensor.dtype, tensor.device))
            checked.append(tensor.contiguous())
        means, covs, grad_log_mass, grad_mean, grad_cov = checked
        if D > self.switching_limits()[0] or N > 256 or G > 256 or B * G > 0x7fffffff:
            raise ValueError("aesmc_amd: switching_collapse_backward takes D <= 8 and at most 256 groups of at most 256 components")
        if not (need_means or need_covs or need_log_weights):
            raise ValueError("aesmc_amd: switching_collapse_backward was asked for nothing")
        log_weights = log_weights.contiguous()
        new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=device)
        out_means = new(*means.shape) if need_means else None
        out_covs = new(*covs.shape) if need_covs else None
        out_weights = new(B, G, N) if need_log_weights else None
        if B * G == 0 or N == 0:
            for value in (out_means, out_covs):
                if value is not None:
                    value.zero_()
            return out_means, out_covs, out_weights
        self._launch(device, self._lib.aesmc_switching_collapse_backward,
                     (_ptr(means), 0 if shared else N * D, _ptr(covs), 0 if shared else N * TD, _ptr(log_weights),
                      _ptr(grad_log_mass), _ptr(grad_mean), _ptr(grad_cov), _ptr(out_weights), _ptr(out_means), _ptr(out_covs),
                      B, G, N, D, self._stream(log_weights)),
                     lambda: 8 * (B * (1 if shared else G) * N * (D + TD) * (1 + (1 if need_means or need_covs else 0)) +
                                  B * G * (2 * N + 1 + D + TD)),
                     (means, covs, log_weights, grad_log_mass, grad_mean, grad_cov, out_means, out_covs, out_weights))
        return out_means, out_covs, out_weights

    # ---- K45, K46 ------------------------------------------------------------------------------
    def switching_statistics_columns(self, latent_dim, observation_dim, masked):
        """F of the [16, F] statistics array (aesmc_switching_statistics_columns; 0 outside the limits)."""
        return int(self._lib.aesmc_switching_statistics_columns(int(latent_dim), int(observation_dim), int(bool(masked))))

    def _switching_statistics_workspace(self, device, D, Dy, masked, block):
        """The per-workgroup partials of K45 / K46, kept per device: two blocks (0: the t = 0 step's, 1: the later steps')
        of aesmc_switching_statistics_workspace_bytes each, which depend on D, Dy and the entry only."""
        if block not in (0, 1):
            raise ValueError("aesmc_amd: a statistics block is 0 (the t = 0 step) or 1 (the later steps), got {!r}".format(block))
        ws_bytes = self._statistics_sizes.get((D, Dy, bool(masked)))
        if ws_bytes is None:
            ws_bytes = self._statistics_sizes[(D, Dy, bool(masked))] = \
                int(self._lib.aesmc_switching_statistics_workspace_bytes(D, Dy, int(masked)))
        key = torch.device(device).index
        held = self._statistics_workspaces.get(key)
        if held is None or held.numel() < 2 * ws_bytes:
            held = self._statistics_workspaces[key] = torch.empty(2 * ws_bytes, dtype=torch.uint8, device=device)
        return held, held.data_ptr() + block * ws_bytes

    def switching_statistics_step(self, observation, regime, mean, cov, num_regimes, previous=None, observed=None, block=0,
                                  accumulate=False):
        """One timestep's contribution to the expected sufficient statistics of a switching model
        (aesmc_switching_moment_statistics, K45; with `observed`, aesmc_switching_masked_moment_statistics, K46), added to
        (`accumulate`) or stored over the per-workgroup partials of `block` (0 or 1: two sets this provider keeps per device).
        observation float32 / float64 [B,Dy]; regime int32 [B,N]; mean float64 [B,N,D], cov float64 [B,N,D(D+1)/2]: the
        smoothed moments of time t; previous: None (the t = 0 form) or (regime_prev int32 [B,N], mean_prev, cov_prev, cross
        float64 [B,N,D,D] with cross[i,l] = Cov(z_{t,i}, z_{t-1,l})); observed: None or torch.bool [B,Dy].  Returns nothing:
        `switching_statistics_finish` reads the block.  A regime or previous regime outside [0, num_regimes) contributes
        nothing and raises FLAG_INDEX_OUT_OF_RANGE.  The launches that share a block share every extent and the entry."""
        _require_hip(observation, "observation")
        tag = _tag(observation, "observation")
        _require_hip(mean, "mean")
        device = observation.device
        if mean.dim() != 3 or mean.dtype != torch.float64 or mean.device != device:
            raise ValueError("aesmc_amd: mean must be [batch_size, num_trajectories, D] float64 on {}, got {} {}".format(
                device, tuple(mean.shape), mean.dtype))
        B, N, D = mean.shape
        TD, M = D * (D + 1) // 2, int(num_regimes)
        if observation.dim() != 2 or observation.size(0) != B:
            raise ValueError("aesmc_amd: observation must be [{}, Dy], got {}".format(B, tuple(observation.shape)))
        Dy = observation.size(1)
        wanted = [(regime, (B, N), torch.int32, "regime"), (cov, (B, N, TD), torch.float64, "cov")]
        if previous is not None:
            if len(previous) != 4:
                raise ValueError("aesmc_amd: previous must be None or (regime_prev, mean_prev, cov_prev, cross)")
            wanted += [(previous[0], (B, N), torch.int32, "regime_prev"), (previous[1], (B, N, D), torch.float64, "mean_prev"),
                       (previous[2], (B, N, TD), torch.float64, "cov_prev"), (previous[3], (B, N, D, D), torch.float64, "cross")]
        for tensor, shape, dtype, what in wanted:      # (on `device`, which is a HIP device: no _require_hip of its own)
            if not torch.is_tensor(tensor) or tensor.shape != shape or tensor.dtype != dtype or tensor.device != device:
                raise ValueError("aesmc_amd: {} must be {} {} on {}".format(what, shape, dtype, device))
        limits = self._statistics_sizes.get("limits")
        if limits is None:
            limits = self._statistics_sizes["limits"] = self.switching_limits()
        max_d, max_dy, max_m = limits
        if not (1 <= D <= max_d and 1 <= Dy <= max_dy and 1 <= M <= max_m and B * N <= 0x7fffffff // (max_d * max_d)):
            raise ValueError("aesmc_amd: switching_statistics_step does not take these operands (see switching_covers)")
        if observed is not None:
            observed = self._switching_observed(observed, B, Dy, device)
        held, workspace = self._switching_statistics_workspace(device, D, Dy, observed is not None, block)
        if B * N == 0:
            return
        observation, regime, mean, cov = observation.contiguous(), regime.contiguous(), mean.contiguous(), cov.contiguous()
        earlier = (None,) * 4 if previous is None else tuple(tensor.contiguous() for tensor in previous)
        head = (tag, _ptr(observation)) + (() if observed is None else (_ptr(observed),))
        args = head + (_ptr(regime),) + tuple(_ptr(tensor) for tensor in earlier) + \
            (_ptr(mean), _ptr(cov), workspace, int(bool(accumulate)), _ptr(self.flags(device)), B, N, M, D, Dy,
             self._stream(mean))
        per_trajectory = 4 + 8 * (D + TD) + (0 if previous is None else 4 + 8 * (D + TD + D * D))
        self._launch(device, self._lib.aesmc_switching_moment_statistics if observed is None else
                     self._lib.aesmc_switching_masked_moment_statistics, args,
                     lambda: B * N * per_trajectory + B * Dy * (observation.element_size() + (0 if observed is None else 1)),
                     (observation, observed, regime, mean, cov, earlier, held),
                     name="switching_statistics_step" if observed is None else "switching_masked_statistics_step")

    def switching_statistics_finish(self, like, batch_size, num_trajectories, latent_dim, observation_dim, masked, block=0):
        """The [16, F] float64 statistics of `block` (aesmc_switching_statistics_finish): the workgroups' partials of the
        `switching_statistics_step` launches into it, added in one fixed order.  like: a tensor on the device (its device
        and stream are used); the extents and `masked` are those of the launches.  A new tensor; zeros without a launch
        where batch_size * num_trajectories is 0."""
        _require_hip(like, "like")
        device = like.device
        B, N, D, Dy = int(batch_size), int(num_trajectories), int(latent_dim), int(observation_dim)
        max_d, max_dy, _ = self.switching_limits()
        if not (B >= 0 and N >= 0 and 1 <= D <= max_d and 1 <= Dy <= max_dy and B * N <= 0x7fffffff // (max_d * max_d)):
            raise ValueError("aesmc_amd: switching_statistics_finish does not take these extents (see switching_covers)")
        columns = self.switching_statistics_columns(D, Dy, masked)
        if B * N == 0:
            return torch.zeros((16, columns), dtype=torch.float64, device=device)
        held, workspace = self._switching_statistics_workspace(device, D, Dy, masked, block)
        out = torch.empty((16, columns), dtype=torch.float64, device=device)
        self._launch(device, self._lib.aesmc_switching_statistics_finish,
                     (workspace, _ptr(out), int(bool(masked)), B, N, D, Dy, self._stream(like)),
                     lambda: 8 * 16 * columns * (1 + min((B * N + 255) // 256, 512)), (held, out),
                     name="switching_statistics_finish")
        return out

    # ---- K37, K38 ------------------------------------------------------------------------------
    def switching_conditional_max_particles(self, latent_dim):
        """The largest K of `switching_conditional_ancestor_index` for a latent of D values, as the library exports it (0
        for a D it does not take)."""
        return int(self._lib.aesmc_switching_conditional_max_particles(int(latent_dim)))

    def switching_conditional_covers(self, observation, num_regimes, latent_dim, observation_dim, num_particles):
        """Whether `switching_conditional_ancestor_index` and `switching_kalman_conditional_step` take a conditional sweep
        like this: what `switching_covers` asks, and at most `switching_conditional_max_particles(latent_dim)` particles."""
        return self.switching_covers(observation, num_regimes, latent_dim, observation_dim, num_particles) and \
            num_particles <= self.switching_conditional_max_particles(latent_dim)

    def switching_conditional_ancestor_index(self, log_w, u, log_Pi, regime_next, factor, lam, state):
        """The ancestors of one step of a conditional Rao-Blackwellised filter (aesmc_switching_conditional_ancestor_index,
        K37): log_w, u float64 [B,K]; log_Pi float64 [M,M]; regime_next int32 [B] (the reference's regime at the step being
        entered); factor [B,D(D+1)/2] and lam [B,D]: `switching_information_step`'s with one trajectory per row, squeezed, or
        both None (no ancestor sampling: slot K-1 keeps ancestor K-1); state: the stored (regime, mean, cov) the weights
        belong to.  Slots 0 .. K-2 draw multinomial ancestors as `conditional_ancestor_index` does, slot K-1 from
        `switching_backward_scores`' scores of that one trajectory.  Returns idx int64 [B,K]."""
        _require_hip(log_w, "log_weight")
        _require_hip(u, "uniforms")
        device = log_w.device
        if log_w.dim() != 2 or log_w.dtype != torch.float64:
            raise ValueError("aesmc_amd: log_weight must be [batch_size, num_particles] float64")
        B, K = log_w.shape
        if tuple(u.shape) != (B, K) or u.dtype != torch.float64 or u.device != device:
            raise ValueError("aesmc_amd: uniforms must be [{}, {}] float64 on {}".format(B, K, device))
        _require_hip(log_Pi, "log_Pi")
        if log_Pi.dim() != 2 or log_Pi.size(0) != log_Pi.size(1) or log_Pi.dtype != torch.float64 or log_Pi.device != device:
            raise ValueError("aesmc_amd: log_Pi must be [M, M] float64 on {}".format(device))
        M = log_Pi.size(0)
        D = state[1].size(-1) if torch.is_tensor(state[1]) and state[1].dim() == 3 else 0
        TD = D * (D + 1) // 2
        regime, mean, cov = self._switching_state(state, B, K, D, device)
        _require_hip(regime_next, "regime_next")
        if tuple(regime_next.shape) != (B,) or regime_next.dtype != torch.int32 or regime_next.device != device:
            raise ValueError("aesmc_amd: regime_next must be [{}] int32 on {}".format(B, device))
        if (factor is None) != (lam is None):
            raise ValueError("aesmc_amd: factor and lam come together")
        if factor is not None:
            for tensor, shape, what in ((factor, (B, TD), "factor"), (lam, (B, D), "lam")):
                _require_hip(tensor, what)
                if tuple(tensor.shape) != shape or tensor.dtype != torch.float64 or tensor.device != device:
                    raise ValueError("aesmc_amd: {} must be {} float64 on {}".format(what, shape, device))
            factor, lam = factor.contiguous(), lam.contiguous()
        max_d, _, max_m = self.switching_limits()
        if not (1 <= D <= max_d and 1 <= M <= max_m and K <= self.switching_conditional_max_particles(D) and
                B * K <= 0x7fffffff // (max_d * (max_d + 1) // 2)):
            raise ValueError("aesmc_amd: switching_conditional_ancestor_index does not take these operands (see "
                             "switching_conditional_covers)")
        log_w, u, log_Pi, regime_next = log_w.contiguous(), u.contiguous(), log_Pi.contiguous(), regime_next.contiguous()
        idx = torch.empty((B, K), dtype=torch.int64, device=device)
        if idx.numel() == 0:
            return idx
        self._launch(device, self._lib.aesmc_switching_conditional_ancestor_index,
                     (_ptr(log_w), _ptr(u), _ptr(log_Pi), _ptr(regime_next), _ptr(factor), _ptr(lam), _ptr(regime),
                      _ptr(mean), _ptr(cov), _ptr(idx), _ptr(self.flags(device)), B, K, M, D, self._stream(log_w)),
                     lambda: B * K * 24 + (B * K * (4 + 8 * (D + TD)) + B * (4 + 8 * (TD + D)) + 8 * M * M
                                           if factor is not None else 0),
                     (log_w, u, log_Pi, regime_next, factor, lam, regime, mean, cov, idx),
                     name="switching_conditional_ancestor_index")
        return idx

    def switching_kalman_conditional_step(self, model, state, index, uniforms, pinned_regime, observation, observed=None):
        """`switching_kalman_step` with the regime of slot K-1 pinned (aesmc_switching_kalman_conditional_step, K38):
        pinned_regime int32 [B], the regime particle (b, K-1) takes in place of its draw.  Returns (regime, mean, cov,
        log_weight [B,K] float64), new tensors; flags and NaNs as `switching_kalman_step`'s, a pinned regime outside [0, M)
        as a stored one.  observed: as `switching_kalman_step`'s (K39 with pinned_regime)."""
        return self._switching_kalman("switching_kalman_conditional_step", self._lib.aesmc_switching_kalman_conditional_step,
                                      "switching_kalman_masked_conditional_step", model, state, index, uniforms, observation,
                                      observed, pinned_regime=pinned_regime, pinned=True)

    # ---- K48, K49 ------------------------------------------------------------------------------
    def switching_lookahead_conditional_max_particles(self, num_regimes, latent_dim, observation_dim):
        """The largest K the fused `switching_lookahead_conditional_ancestor_index` (K48) takes for a model of M regimes, a
        latent of D and an observation of Dy values, as the library exports it (0 outside the family's limits); never above
        `switching_conditional_max_particles(latent_dim)`."""
        return int(self._lib.aesmc_switching_lookahead_conditional_max_particles(int(num_regimes), int(latent_dim),
                                                                                 int(observation_dim)))

    def switching_lookahead_conditional_covers(self, observation, num_regimes, latent_dim, observation_dim, num_particles):
        """Whether ONE launch (K48) takes the resampling side of a look-ahead conditional step like this: what
        `switching_conditional_covers` asks, and at most `switching_lookahead_conditional_max_particles` particles.  Past it
        and inside `switching_conditional_covers` the step is composed from K32 and K37."""
        return self.switching_conditional_covers(observation, num_regimes, latent_dim, observation_dim, num_particles) and \
            num_particles <= self.switching_lookahead_conditional_max_particles(num_regimes, latent_dim, observation_dim)

    def switching_lookahead_conditional_ancestor_index(self, model, log_Pi, state, observation, u, regime_next, factor, lam,
                                                       observed=None, fused=None):
        """The resampling side of one step t >= 1 of a LOOK-AHEAD conditional sweep: `switching_lookahead` on the stored,
        equally weighted system `state` with log_Pi as its log-prior, and `switching_conditional_ancestor_index` on the
        first-stage log-weights it gives — with the pinned slot's score carrying a log-weight of 0.0, NOT the first-stage
        weight.  model, state, observation, observed as `switching_lookahead`'s; u float64 [B,K]; regime_next int32 [B];
        factor, lam as `switching_conditional_ancestor_index`'s, or both None (no ancestor sampling).
        fused: None — one launch (aesmc_switching_lookahead_conditional_ancestor_index, K48; with `observed` its masked
        entry) where `switching_lookahead_conditional_covers` holds, else the composition of existing launches: K32 (K40),
        K37 on the first-stage weights without factor / lam for columns 0 .. K-2, K37 on zeros with them for column K-1, one
        torch.where; True / False force either (True past the cap raises).
        Returns (idx int64 [B,K], log_weight [B,K], cdf [B,K,M]) float64, new tensors.  Bad rows as the two functions'."""
        _require_hip(observation, "observation")
        tag = _tag(observation, "observation")
        device = observation.device
        block, M, D, Dy = self._switching_block(model, device)
        _require_hip(u, "uniforms")
        if u.dim() != 2 or u.dtype != torch.float64 or u.device != device:
            raise ValueError("aesmc_amd: uniforms must be [batch_size, num_particles] float64 on {}".format(device))
        B, K = u.shape
        if tuple(observation.shape) != (B, Dy):
            raise ValueError("aesmc_amd: observation must be [{}, {}], got {}".format(B, Dy, tuple(observation.shape)))
        if state is None:
            raise ValueError("aesmc_amd: switching_lookahead_conditional_ancestor_index covers later steps only: step 0 has "
                             "no resampling (switching_lookahead on the prior)")
        if not self.switching_conditional_covers(observation, M, D, Dy, K):
            raise ValueError("aesmc_amd: switching_lookahead_conditional_ancestor_index does not take these operands (see "
                             "switching_conditional_covers)")
        covered = K <= self.switching_lookahead_conditional_max_particles(M, D, Dy)
        if fused and not covered:
            raise ValueError("aesmc_amd: fused=True with {} particles, above switching_lookahead_conditional_max_particles({}, "
                             "{}, {})".format(K, M, D, Dy))
        if not (covered if fused is None else fused):
            return compose_switching_lookahead_conditional(self, model, log_Pi, state, observation, u, regime_next, factor,
                                                           lam, observed)
        _require_hip(log_Pi, "log_Pi")
        if tuple(log_Pi.shape) != (M, M) or log_Pi.dtype != torch.float64 or log_Pi.device != device:
            raise ValueError("aesmc_amd: log_Pi must be {} float64 on {}".format((M, M), device))
        TD = D * (D + 1) // 2
        regime, mean, cov = self._switching_state(state, B, K, D, device)
        if (factor is None) != (lam is None):
            raise ValueError("aesmc_amd: factor and lam come together")
        if factor is not None:
            for tensor, shape, what in ((factor, (B, TD), "factor"), (lam, (B, D), "lam")):
                _require_hip(tensor, what)
                if tuple(tensor.shape) != shape or tensor.dtype != torch.float64 or tensor.device != device:
                    raise ValueError("aesmc_amd: {} must be {} float64 on {}".format(what, shape, device))
            factor, lam = factor.contiguous(), lam.contiguous()
        _require_hip(regime_next, "regime_next")
        if tuple(regime_next.shape) != (B,) or regime_next.dtype != torch.int32 or regime_next.device != device:
            raise ValueError("aesmc_amd: regime_next must be [{}] int32 on {}".format(B, device))
        log_Pi, u, regime_next, observation = log_Pi.contiguous(), u.contiguous(), regime_next.contiguous(), \
            observation.contiguous()
        if observed is not None:
            observed = self._switching_observed(observed, B, Dy, device)
        idx = torch.empty((B, K), dtype=torch.int64, device=device)
        log_weight = torch.empty((B, K), dtype=torch.float64, device=device)
        cdf = torch.empty((B, K, M), dtype=torch.float64, device=device)
        if idx.numel() == 0:
            return idx, log_weight, cdf
        head = (tag, ctypes.byref(block), _ptr(log_Pi), _ptr(regime), _ptr(mean), _ptr(cov), _ptr(observation))
        tail = (_ptr(u), _ptr(regime_next), _ptr(factor), _ptr(lam), _ptr(idx), _ptr(log_weight), _ptr(cdf),
                _ptr(self.flags(device)), B, K, self._stream(observation))
        masked = observed is not None
        self._launch(device, self._lib.aesmc_switching_masked_lookahead_conditional_ancestor_index if masked else
                     self._lib.aesmc_switching_lookahead_conditional_ancestor_index,
                     head + (_ptr(observed),) + tail if masked else head + tail,
                     lambda: B * K * (4 + 8 * D + 8 * TD + 8 + 8 * M + 16) + B * Dy * (observation.element_size() + int(masked)) +
                     self._switching_model_bytes(M, D, Dy) + (B * (4 + 8 * (TD + D)) if factor is not None else 0),
                     (model, log_Pi, regime, mean, cov, observation, observed, u, regime_next, factor, lam, idx, log_weight, cdf,
                      block), name="switching_masked_lookahead_conditional_ancestor_index" if masked else
                     "switching_lookahead_conditional_ancestor_index")
        return idx, log_weight, cdf

    def switching_kalman_conditional_draw(self, model, state, index, uniforms, cdf, pinned_regime, observation, observed=None):
        """`switching_kalman_draw` with the regime of slot K-1 pinned (aesmc_switching_kalman_conditional_draw, K49): the
        step of a look-ahead conditional sweep.  cdf float64 [B,K,M] as `switching_kalman_draw`'s, pinned_regime int32 [B] as
        `switching_kalman_conditional_step`'s.  Returns (regime, mean, cov, log_likelihood [B,K] float64), new tensors;
        observed: as `switching_kalman_step`'s (K39 with both operands)."""
        return self._switching_kalman("switching_kalman_conditional_draw", self._lib.aesmc_switching_kalman_conditional_draw,
                                      "switching_kalman_masked_conditional_draw", model, state, index, uniforms, observation,
                                      observed, cdf=cdf, pinned_regime=pinned_regime, draw=True, pinned=True)

    # ---- K22 -----------------------------------------------------------------------------------
    PAIRWISE_LSE_MAX_DIM = 256

    @staticmethod
    def pairwise_lse_covers(rows, cols, scale, col_a, col_sub=None, row_add=None):
        """Whether `pairwise_lse` takes these operands: float32 / float64 throughout and all on one device, rows [B,R,*]
        and cols [B,C,*] with the same trailing dims of at most 256 values (none: no distance term, scale may be None), at
        least one column, a scale of one value or one per value, col_a / col_sub [B,C] and row_add [B,R]."""
        if not (torch.is_tensor(col_a) and col_a.dim() == 2 and col_a.dtype in _DTYPE_TAG and col_a.size(1) > 0):
            return False
        same = lambda t: torch.is_tensor(t) and t.dtype == col_a.dtype and t.device == col_a.device
        if not (same(rows) and same(cols) and rows.dim() >= 2 and cols.dim() == rows.dim() and
                rows.size(0) == col_a.size(0) and tuple(cols.shape[:2]) == tuple(col_a.shape) and
                tuple(cols.shape[2:]) == tuple(rows.shape[2:])):
            return False
        if col_sub is not None and not (same(col_sub) and tuple(col_sub.shape) == tuple(col_a.shape)):
            return False
        if row_add is not None and not (same(row_add) and tuple(row_add.shape) == tuple(rows.shape[:2])):
            return False
        D = 1
        for size in rows.shape[2:]:
            D *= size
        if D == 0:
            return scale is None or same(scale)
        return D <= HipKernels.PAIRWISE_LSE_MAX_DIM and same(scale) and scale.dim() <= 1 and scale.numel() in (1, D)

    def pairwise_lse(self, rows, cols, scale, col_a, col_sub=None, row_add=None):
        """The pairwise Gaussian log-sum-exp (aesmc_pairwise_lse, K22):
            out[b,r] = row_add[b,r] + log sum_c exp(col_a[b,c] - col_sub[b,c] - 1/2 sum_d ((rows[b,r,d] - cols[b,c,d]) / scale[d])^2)
        rows [B,R,*], cols [B,C,*] (trailing dims flattened; a [B,R] tensor has one value per point, a [B,R,0] one none:
        no distance term), scale one value or one per value, col_a / col_sub [B,C], row_add [B,R]; col_sub / row_add None:
        0.  Returns [B,R] in col_a's dtype.  Views are taken as they are (element strides)."""
        tag = self._rows_operand(col_a, "col_a")
        if not self.pairwise_lse_covers(rows, cols, scale, col_a, col_sub, row_add):
            raise ValueError("aesmc_amd: pairwise_lse does not take these operands (see pairwise_lse_covers)")
        B, C = col_a.shape
        R = rows.size(1)
        for t in (rows, cols, col_sub, row_add):
            if t is not None:
                _require_hip(t, "pairwise operand")
        col_a = col_a.contiguous()
        col_sub = None if col_sub is None else col_sub.contiguous()
        row_add = None if row_add is None else row_add.contiguous()
        out = torch.empty((B, R), dtype=col_a.dtype, device=col_a.device)
        if out.numel() == 0:
            return out
        views, keep, D, scale_stride = [None, None], [rows, cols], 0, 0
        if all(size > 0 for size in rows.shape[2:]):
            (rows, sr, D), (cols, sc, _) = self._view3(rows), self._view3(cols)
            _require_hip(scale, "scale")
            scale = scale.reshape(-1).contiguous()
            scale_stride = 0 if scale.numel() == 1 else 1
            views = [_lib.View3(_ptr(rows), *sr), _lib.View3(_ptr(cols), *sc)]
            keep = [rows, cols, scale]
        esz = col_a.element_size()
        refs = [ctypes.byref(v) if v is not None else None for v in views]
        self._launch(col_a.device, self._lib.aesmc_pairwise_lse,
                     (tag, refs[0], refs[1], _ptr(scale) if D else 0, scale_stride, _ptr(col_a), _ptr(col_sub),
                      _ptr(row_add), _ptr(out), _ptr(self.flags(col_a.device)), B, R, C, D, self._stream(col_a)),
                     lambda: B * esz * ((R + C) * D + C * (2 if col_sub is not None else 1) +
                                        R * (2 if row_add is not None else 1)),
                     tuple(keep) + (col_a, col_sub, row_add, out) + tuple(views))
        return out

    # ---- K23 -----------------------------------------------------------------------------------
    PAIRWISE_MEAN_MAX_PAYLOAD = 256

    @staticmethod
    def pairwise_mean_covers(rows, cols, scale, col_a, payload, col_sub=None, row_add=None):
        """Whether `pairwise_mean` takes these operands: what `pairwise_lse_covers` takes, and a payload [B,C,*] of the same
        dtype on the same device with 1 .. 256 values per column (a [B,C] payload has one)."""
        if not HipKernels.pairwise_lse_covers(rows, cols, scale, col_a, col_sub, row_add):
            return False
        if not (torch.is_tensor(payload) and payload.dtype == col_a.dtype and payload.device == col_a.device and
                payload.dim() >= 2 and tuple(payload.shape[:2]) == tuple(col_a.shape)):
            return False
        P = 1
        for size in payload.shape[2:]:
            P *= size
        return 1 <= P <= HipKernels.PAIRWISE_MEAN_MAX_PAYLOAD

    def pairwise_mean(self, rows, cols, scale, col_a, payload, col_sub=None, row_add=None):
        """The pairwise Gaussian softmax mean (aesmc_pairwise_mean, K23), with s[b,r,c] the score `pairwise_lse` sums:
            out[b,r,p] = sum_c softmax_c(s[b,r,:])[c] * payload[b,c,p]
            lse[b,r]   = pairwise_lse(rows, cols, scale, col_a, col_sub, row_add)[b,r]
        Operands as `pairwise_lse` takes them; payload [B,C,*] (trailing dims flattened to P <= 256 values).  Returns
        (out [B,R,P], lse [B,R]) in col_a's dtype.  Views are taken as they are (element strides)."""
        tag = self._rows_operand(col_a, "col_a")
        if not self.pairwise_mean_covers(rows, cols, scale, col_a, payload, col_sub, row_add):
            raise ValueError("aesmc_amd: pairwise_mean does not take these operands (see pairwise_mean_covers)")
        B, C = col_a.shape
        R = rows.size(1)
        for t in (rows, cols, payload, col_sub, row_add):
            if t is not None:
                _require_hip(t, "pairwise operand")
        col_a = col_a.contiguous()
        col_sub = None if col_sub is None else col_sub.contiguous()
        row_add = None if row_add is None else row_add.contiguous()
        payload, sp, P = self._view3(payload)
        out = torch.empty((B, R, P), dtype=col_a.dtype, device=col_a.device)
        lse = torch.empty((B, R), dtype=col_a.dtype, device=col_a.device)
        if lse.numel() == 0:
            return out, lse
        views, keep, D, scale_stride = [None, None], [rows, cols], 0, 0
        if all(size > 0 for size in rows.shape[2:]):
            (rows, sr, D), (cols, sc, _) = self._view3(rows), self._view3(cols)
            _require_hip(scale, "scale")
            scale = scale.reshape(-1).contiguous()
            scale_stride = 0 if scale.numel() == 1 else 1
            views = [_lib.View3(_ptr(rows), *sr), _lib.View3(_ptr(cols), *sc)]
            keep = [rows, cols, scale]
        views.append(_lib.View3(_ptr(payload), *sp))
        esz = col_a.element_size()
        refs = [ctypes.byref(v) if v is not None else None for v in views]
        self._launch(col_a.device, self._lib.aesmc_pairwise_mean,
                     (tag, refs[0], refs[1], _ptr(scale) if D else 0, scale_stride, _ptr(col_a), _ptr(col_sub),
                      _ptr(row_add), refs[2], _ptr(out), _ptr(lse), _ptr(self.flags(col_a.device)), B, R, C, D, P,
                      self._stream(col_a)),
                     lambda: B * esz * ((R + C) * D + C * P + R * P + C * (2 if col_sub is not None else 1) +
                                        R * (2 if row_add is not None else 1)),
                     tuple(keep) + (col_a, col_sub, row_add, payload, out, lse) + tuple(views))
        return out, lse

    # ---- K24 -----------------------------------------------------------------------------------
    PAIRWISE_ARGMAX_MAX_DIM = 256

    @staticmethod
    def pairwise_argmax_covers(rows, cols, scale, col_a, col_sub=None, row_add=None):
        """Whether `pairwise_argmax` takes these operands: what `pairwise_lse_covers` takes."""
        return HipKernels.pairwise_lse_covers(rows, cols, scale, col_a, col_sub, row_add)

    def pairwise_argmax(self, rows, cols, scale, col_a, col_sub=None, row_add=None):
        """The pairwise Gaussian max and argmax (aesmc_pairwise_argmax, K24), with s[b,r,c] the score `pairwise_lse` sums:
            out[b,r] = row_add[b,r] + max_c s[b,r,c]          arg[b,r] = the smallest c that attains the maximum
        Operands as `pairwise_lse` takes them.  Returns (out [B,R] in col_a's dtype, arg int64 [B,R]); arg == C: no column
        (a NaN, a +inf or an all -inf row point).  Views are taken as they are (element strides)."""
        tag = self._rows_operand(col_a, "col_a")
        if not self.pairwise_argmax_covers(rows, cols, scale, col_a, col_sub, row_add):
            raise ValueError("aesmc_amd: pairwise_argmax does not take these operands (see pairwise_argmax_covers)")
        B, C = col_a.shape
        R = rows.size(1)
        for t in (rows, cols, col_sub, row_add):
            if t is not None:
                _require_hip(t, "pairwise operand")
        col_a = col_a.contiguous()
        col_sub = None if col_sub is None else col_sub.contiguous()
        row_add = None if row_add is None else row_add.contiguous()
        out = torch.empty((B, R), dtype=col_a.dtype, device=col_a.device)
        arg = torch.empty((B, R), dtype=torch.int64, device=col_a.device)
        if out.numel() == 0:
            return out, arg
        views, keep, D, scale_stride = [None, None], [rows, cols], 0, 0
        if all(size > 0 for size in rows.shape[2:]):
            (rows, sr, D), (cols, sc, _) = self._view3(rows), self._view3(cols)
            _require_hip(scale, "scale")
            scale = scale.reshape(-1).contiguous()
            scale_stride = 0 if scale.numel() == 1 else 1
            views = [_lib.View3(_ptr(rows), *sr), _lib.View3(_ptr(cols), *sc)]
            keep = [rows, cols, scale]
        esz = col_a.element_size()
        refs = [ctypes.byref(v) if v is not None else None for v in views]
        self._launch(col_a.device, self._lib.aesmc_pairwise_argmax,
                     (tag, refs[0], refs[1], _ptr(scale) if D else 0, scale_stride, _ptr(col_a), _ptr(col_sub),
                      _ptr(row_add), _ptr(out), _ptr(arg), _ptr(self.flags(col_a.device)), B, R, C, D,
                      self._stream(col_a)),
                     lambda: B * esz * ((R + C) * D + C * (2 if col_sub is not None else 1) +
                                        R * (2 if row_add is not None else 1)) + 8 * B * R,
                     tuple(keep) + (col_a, col_sub, row_add, out, arg) + tuple(views))
        return out, arg

    # ---- K25 -----------------------------------------------------------------------------------
    PAIRWISE_PASS_MAX_DIM = 256

    @staticmethod
    def pairwise_pass_covers(own, others, scale, own_term, other_term, own_gain=None, other_gain=None):
        """Whether `pairwise_pass` takes these operands: float32 / float64 throughout and all on one device, own [B,N,*]
        and others [B,M,*] with the same trailing dims of at most 256 values (none: no distance term, scale may be None), at
        least one other, a scale of one value or one per value, own_term / own_gain [B,N] and other_term / other_gain
        [B,M]."""
        if not (torch.is_tensor(own_term) and own_term.dim() == 2 and own_term.dtype in _DTYPE_TAG):
            return False
        same = lambda t: torch.is_tensor(t) and t.dtype == own_term.dtype and t.device == own_term.device
        if not (same(other_term) and other_term.dim() == 2 and other_term.size(0) == own_term.size(0) and
                other_term.size(1) > 0):
            return False
        if not (same(own) and same(others) and own.dim() >= 2 and others.dim() == own.dim() and
                tuple(own.shape[:2]) == tuple(own_term.shape) and tuple(others.shape[:2]) == tuple(other_term.shape) and
                tuple(others.shape[2:]) == tuple(own.shape[2:])):
            return False
        if own_gain is not None and not (same(own_gain) and tuple(own_gain.shape) == tuple(own_term.shape)):
            return False
        if other_gain is not None and not (same(other_gain) and tuple(other_gain.shape) == tuple(other_term.shape)):
            return False
        D = 1
        for size in own.shape[2:]:
            D *= size
        if D == 0:
            return scale is None or same(scale)
        return D <= HipKernels.PAIRWISE_PASS_MAX_DIM and same(scale) and scale.dim() <= 1 and scale.numel() in (1, D)

    def pairwise_pass(self, own, others, scale, own_term, other_term, own_gain=None, other_gain=None, want_mass=True,
                      want_pull=True, want_spread=True):
        """The pairwise Gaussian weighted pass (aesmc_pairwise_pass, K25), the backward of `pairwise_lse`:
            w[n,m]        = exp(own_term[b,n] + other_term[b,m] - 1/2 sum_d ((own[b,n,d] - others[b,m,d]) / scale[d])^2)
                            * own_gain[b,n] * other_gain[b,m]
            mass[b,n]     = sum_m w[n,m]
            pull[b,n,d]   = sum_m w[n,m] (others[b,m,d] - own[b,n,d]) / scale[d]^2
            spread[b,n,d] = sum_m w[n,m] ((own[b,n,d] - others[b,m,d]) / scale[d])^2
        own [B,N,*], others [B,M,*] (trailing dims flattened; a [B,N,0] tensor: no distance term, mass only), scale one
        value or one per value, own_term / own_gain [B,N], other_term / other_gain [B,M]; a gain of None: 1.  Returns
        (mass [B,N], pull [B,N,D], spread [B,N,D]) in own_term's dtype, None for what was not wanted.  Views are taken as
        they are (element strides)."""
        tag = self._rows_operand(own_term, "own_term")
        if not self.pairwise_pass_covers(own, others, scale, own_term, other_term, own_gain, other_gain):
            raise ValueError("aesmc_amd: pairwise_pass does not take these operands (see pairwise_pass_covers)")
        (B, N), M = own_term.shape, other_term.size(1)
        for t in (own, others, other_term, own_gain, other_gain):
            if t is not None:
                _require_hip(t, "pairwise operand")
        own_term, other_term = own_term.contiguous(), other_term.contiguous()
        own_gain = None if own_gain is None else own_gain.contiguous()
        other_gain = None if other_gain is None else other_gain.contiguous()
        views, keep, D, scale_stride = [None, None], [own, others], 0, 0
        if all(size > 0 for size in own.shape[2:]):
            (own, so, D), (others, st, _) = self._view3(own), self._view3(others)
            _require_hip(scale, "scale")
            scale = scale.reshape(-1).contiguous()
            scale_stride = 0 if scale.numel() == 1 else 1
            views = [_lib.View3(_ptr(own), *so), _lib.View3(_ptr(others), *st)]
            keep = [own, others, scale]
        new = lambda *shape: torch.empty(shape, dtype=own_term.dtype, device=own_term.device)
        mass = new(B, N) if want_mass else None
        pull = new(B, N, D) if want_pull else None
        spread = new(B, N, D) if want_spread else None
        if B * N == 0 or not (want_mass or (D > 0 and (want_pull or want_spread))):
            return mass, pull, spread
        esz = own_term.element_size()
        refs = [ctypes.byref(v) if v is not None else None for v in views]
        self._launch(own_term.device, self._lib.aesmc_pairwise_pass,
                     (tag, refs[0], refs[1], _ptr(scale) if D else 0, scale_stride, _ptr(own_term), _ptr(other_term),
                      _ptr(own_gain), _ptr(other_gain), _ptr(mass), _ptr(pull) if D else 0, _ptr(spread) if D else 0,
                      _ptr(self.flags(own_term.device)), B, N, M, D, self._stream(own_term)),
                     lambda: B * esz * ((N + M) * D + N * (1 if own_gain is None else 2) + M * (1 if other_gain is None else 2) +
                                        N * ((1 if want_mass else 0) + D * ((1 if want_pull else 0) + (1 if want_spread else 0)))),
                     tuple(keep) + (own_term, other_term, own_gain, other_gain, mass, pull, spread) + tuple(views))
        return mass, pull, spread



_provider = None
_provider_lock = threading.Lock()


def get():
    """The active kernel provider (created on first use; raises if the library is missing)."""
    global _provider
    if _provider is None:
        with _provider_lock:
            if _provider is None:
                _provider = HipKernels()
    return _provider


def compose_switching_lookahead_conditional(provider, model, log_Pi, state, observation, u, regime_next, factor, lam,
                                            observed=None):
    """`switching_lookahead_conditional_ancestor_index` from a provider's existing launches: K32 (with `observed` K40), K37 on
    the first-stage weights without factor / lam for columns 0 .. K-2, and with ancestor sampling K37 on zeros with them for
    column K-1, joined by one torch.where.  Returns (idx, log_weight, cdf)."""
    mask = {} if observed is None else {"observed": observed}
    log_weight, cdf = provider.switching_lookahead(model, log_Pi, state, observation, **mask)
    idx = provider.switching_conditional_ancestor_index(log_weight, u, log_Pi, regime_next, None, None, state)
    if factor is not None or lam is not None:
        pinned = provider.switching_conditional_ancestor_index(torch.zeros_like(log_weight), u, log_Pi, regime_next, factor,
                                                               lam, state)
        # (column K-1 of the first is K-1, or K where the row's first-stage weights are bad: those rows stay)
        K = idx.size(1)
        last = torch.arange(K, device=idx.device) == K - 1
        idx = torch.where(last & (idx == K - 1), pinned, idx)
    return idx, log_weight, cdf


def _swap_provider_for_tests(provider):
    """Test hook (used by tests/conftest.py only): substitute the kernel provider so the host
    logic can be exercised on CPU tensors against the oracle.  Returns the previous provider."""
    global _provider
    previous, _provider = _provider, provider
    return previous
