"""
The reconstruction SDR of reference ``experiments/evaluate.py:40,51,122-127``, which delegates to
``torchmetrics.audio.SignalDistortionRatio()`` (defaults); the package is absent from this image.  ``signal_distortion_ratio`` restates
its published algorithm (the filtered SDR of Scheibler 2021, "SDR -- medium rare with fast computations", as implemented by torchmetrics
/ fast_bss_eval) on the host in float64.  PARITY UNPINNED against the package itself (it is not installed and there is no network);
pinned instead by known-answer tests (tests/test_metrics.py) and by an independent dense least-squares derivation of the same quantity.

``signal_distortion_ratio_device`` / ``SignalDistortionRatio`` compute the same SDR where ``evaluate.py`` asks for it -- on the device,
right after ``sliCQ.decode`` -- in float64 HIP kernels (csrc/sdr.hip: direct correlation sums and a Levinson recursion instead of FFTs
and a dense solve); ``signal_distortion_ratio`` stays the float64 yardstick they are tested against.
"""

import numpy as np
import torch

from ... import _hip


def _next_pow2(n):
    return 1 << int(np.ceil(np.log2(max(int(n), 1))))


def signal_distortion_ratio(preds, target, filter_length=512, zero_mean=False, load_diag=None):
    """
    Signal-to-distortion ratio in dB, the distortion being what is left of ``preds`` after projection onto the span of
    ``filter_length`` delayed copies of ``target`` (BSS-eval's SDR, computed the fast way):

        both signals scaled to unit norm;  r = autocorrelation of target (lags 0 .. L-1),  b = cross-correlation target -> preds;
        solve  Toeplitz(r) h = b ;   coherence = b . h ;   SDR = 10 log10(coherence / (1 - coherence)).

    ``preds`` / ``target``: arrays or tensors (..., time); float64 throughout; returns an ndarray of the leading shape (a float
    for 1-D input).  Mirrors ``torchmetrics.functional.audio.signal_distortion_ratio`` with its defaults (dense solve).
    """
    p = np.asarray(preds.detach().cpu() if hasattr(preds, 'detach') else preds, dtype=np.float64)
    t = np.asarray(target.detach().cpu() if hasattr(target, 'detach') else target, dtype=np.float64)
    if p.shape != t.shape:
        raise ValueError('preds and target must have the same shape')
    if zero_mean:
        p = p - p.mean(axis=-1, keepdims=True)
        t = t - t.mean(axis=-1, keepdims=True)
    t = t / np.maximum(np.linalg.norm(t, axis=-1, keepdims=True), 1e-6)
    p = p / np.maximum(np.linalg.norm(p, axis=-1, keepdims=True), 1e-6)
    n_fft = _next_pow2(p.shape[-1] + t.shape[-1] - 1)
    tf = np.fft.rfft(t, n=n_fft, axis=-1)
    r0 = np.fft.irfft(tf.real ** 2 + tf.imag ** 2, n=n_fft, axis=-1)[..., :filter_length]
    b = np.fft.irfft(np.conj(tf) * np.fft.rfft(p, n=n_fft, axis=-1), n=n_fft, axis=-1)[..., :filter_length]
    if load_diag is not None:
        r0 = r0.copy()
        r0[..., 0] += load_diag
    lead = r0.shape[:-1]
    r0f, bf = r0.reshape(-1, filter_length), b.reshape(-1, filter_length)
    idx = np.abs(np.subtract.outer(np.arange(filter_length), np.arange(filter_length)))
    out = np.empty(r0f.shape[0])
    for i in range(r0f.shape[0]):
        sol = np.linalg.solve(r0f[i][idx], bf[i])
        coh = float(np.dot(bf[i], sol))
        ratio = coh / (1.0 - coh)
        out[i] = 10.0 * np.log10(ratio) if ratio > 0 else -np.inf
    return float(out[0]) if not lead else out.reshape(lead)


# ---- on the device (csrc/sdr.hip) ----------------------------------------------------------------------------------------

SDR_CHUNK = 8192          # samples per workgroup of the correlation kernel (= tt_sdr_chunk(), checked on first use)
SDR_MAX_FILTER = 512      # largest filter_length the kernels hold in LDS


def _sdr_check(preds, target, filter_length):
    _hip.require_cuda(preds, target)
    if preds.shape != target.shape:
        raise ValueError('preds and target must have the same shape (got %s and %s)' % (tuple(preds.shape), tuple(target.shape)))
    if preds.dim() < 1 or preds.shape[-1] < 1:
        raise ValueError('preds and target must be (..., time) with at least one sample')
    if int(filter_length) != filter_length or not 1 <= filter_length <= SDR_MAX_FILTER:
        raise ValueError('filter_length must be an integer in [1, %d] (got %r)' % (SDR_MAX_FILTER, filter_length))
    for x in (preds, target):
        if x.dtype == torch.float64:
            raise ValueError('signal_distortion_ratio_device takes fp32 / fp16 / bf16 tensors; float64 input is what the host '
                             'function signal_distortion_ratio is for')
        if x.dtype not in (torch.float32, torch.float16, torch.bfloat16):
            raise ValueError('unsupported dtype %s' % x.dtype)
    lib = _hip.lib()
    if lib.tt_sdr_chunk() != SDR_CHUNK:
        raise RuntimeError('libttrap_hip.so was built with a chunk of %d samples, metrics.SDR_CHUNK says %d' % (lib.tt_sdr_chunk(), SDR_CHUNK))
    return lib


def sdr_correlations(preds, target, filter_length=512, zero_mean=False):
    """
    The un-normalised sums the device SDR rests on: a float64 device tensor (B, 2 L + 1) holding, per clip of the flattened
    leading shape, r[0..L) (autocorrelation of ``target``), b[0..L) (cross-correlation target -> preds) and sum(preds^2),
    all linear (zeros beyond the clip's end), of the signals minus their means when ``zero_mean``.
    """
    lib = _sdr_check(preds, target, filter_length)
    L, N = int(filter_length), preds.shape[-1]
    p = preds.reshape(-1, N).float().contiguous()
    t = target.reshape(-1, N).float().contiguous()
    B = p.shape[0]
    if B < 1:
        raise ValueError('preds and target hold no clip')
    scratch = torch.empty(lib.tt_sdr_scratch_bytes(B, N, L) // 8, dtype=torch.float64, device=p.device)
    rb = torch.empty(B, 2 * L + 1, dtype=torch.float64, device=p.device)
    means = None
    with torch.cuda.device(p.device):
        st = _hip.stream_ptr()
        if zero_mean:
            means = torch.empty(B, 2, dtype=torch.float64, device=p.device)
            _hip.check(lib.tt_sdr_means(_hip.ptr(p), _hip.ptr(t), B, N, _hip.ptr(scratch), _hip.ptr(means), st), 'tt_sdr_means')
        _hip.check(lib.tt_sdr_correlate(_hip.ptr(p), _hip.ptr(t), B, N, L, _hip.ptr(means), _hip.ptr(scratch), _hip.ptr(rb), st),
                   'tt_sdr_correlate')
    return rb


def signal_distortion_ratio_device(preds, target, filter_length=512, zero_mean=False, load_diag=None):
    """
    ``signal_distortion_ratio`` for device tensors (..., N) of equal shape, computed where they are: a float64 device tensor
    of the leading shape, launched on the current stream without a host synchronisation (reference
    ``experiments/evaluate.py:51,122-127``).  fp16 / bf16 inputs are upcast to fp32; float64 raises ``ValueError`` (use the
    host function); CPU tensors raise ``RuntimeError`` -- there is no CPU fallback.  ``filter_length`` <= 512.

    Agreement with the host function: the correlations are direct float64 sums of exact products instead of FFTs, the solve
    is a Levinson recursion instead of a dense one; measured <= 5e-9 dB in float64 up to a Toeplitz condition number of 4e11.
    The one difference: an all-zero ``target`` gives a non-finite value here, where the host function raises ``LinAlgError``.
    """
    rb = sdr_correlations(preds, target, filter_length, zero_mean)
    B, L = rb.shape[0], int(filter_length)
    out = torch.empty(2, B, dtype=torch.float64, device=rb.device)
    with torch.cuda.device(rb.device):
        _hip.check(_hip.lib().tt_sdr_finish(_hip.ptr(rb), B, L, 0.0 if load_diag is None else float(load_diag), int(load_diag is not None),
                                            _hip.ptr(out[0]), _hip.ptr(out[1]), _hip.stream_ptr()), 'tt_sdr_finish')
    return out[1].reshape(preds.shape[:-1])


class SignalDistortionRatio(torch.nn.Module):
    """
    The call shape of ``torchmetrics.audio.SignalDistortionRatio`` as ``experiments/evaluate.py:51,122-127`` uses it:
    ``SignalDistortionRatio().to(device)``, then ``module(preds, target)`` -> the mean SDR over all clips of the batch as a
    0-dim tensor in ``preds``' dtype (``.item()`` is the caller's one host sync).  ``forward`` and ``update`` also add the
    batch to a running sum (float64, on the inputs' device) and count; ``compute`` is their ratio, ``reset`` clears them.
    """

    def __init__(self, filter_length=512, zero_mean=False, load_diag=None):
        super().__init__()
        self.filter_length, self.zero_mean, self.load_diag = filter_length, zero_mean, load_diag
        self.reset()

    def reset(self):
        self.sum_sdr, self.total = None, 0

    def _accumulate(self, preds, target):
        values = signal_distortion_ratio_device(preds, target, self.filter_length, self.zero_mean, self.load_diag)
        batch = values.sum()
        self.sum_sdr = batch if self.sum_sdr is None else self.sum_sdr + batch
        self.total += values.numel()
        return values

    def update(self, preds, target):
        self._accumulate(preds, target)

    def forward(self, preds, target):
        return self._accumulate(preds, target).mean().to(preds.dtype)

    def compute(self):
        if self.total == 0:
            raise RuntimeError('SignalDistortionRatio.compute() before any update()')
        return self.sum_sdr / self.total
