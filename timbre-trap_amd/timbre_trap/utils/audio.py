"""
Track audio in front of the hot path: what reference ``timbre_trap/datasets/AudioDataset.py:69-77`` (``AudioDataset.get_audio``)
does to a decoded file before anything else sees it --

    audio = torch.mean(audio, dim=0, keepdim=True)                        # mono mix
    audio = torchaudio.functional.resample(audio, fs, self.sample_rate)   # 44.1 / 48 / 16 kHz -> 22.05 kHz
    if audio.abs().max(): audio /= audio.abs().max()                      # inf-norm

-- on the device (csrc/resample.hip): ``resample`` has the signature of ``torchaudio.functional.resample``, ``prepare_audio`` is the
three lines in two launches (mix + polyphase FIR + per-workgroup peaks, then the division).  ``resample_host`` is the float64
yardstick on the CPU the kernels are tested against: the same fp32 taps, accumulated in float64.  File decoding
(``torchaudio.load``) stays host work.

The taps are torchaudio's windowed-sinc design (``sinc_interp_hann``), restated from its published source in
``sinc_resample_kernel``.  PARITY UNPINNED against torchaudio itself (it is not installed here); pinned instead by the tap-table
dimensions, the unit DC gain of every phase, impulse responses and a known-answer sine (tests/test_resample_restatement.py).
"""

import functools
import math

import numpy as np
import torch

from .. import _hip

__all__ = ['sinc_resample_kernel', 'resample_host', 'resample', 'mix_resample', 'prepare_audio', 'resample_tiles']


def _reduced(orig_freq, new_freq):
    if int(orig_freq) != orig_freq or int(new_freq) != new_freq:
        raise ValueError('resampling takes integer sample rates (got %r -> %r); scale both to integers with the same ratio'
                         % (orig_freq, new_freq))
    orig_freq, new_freq = int(orig_freq), int(new_freq)
    if orig_freq <= 0 or new_freq <= 0:
        raise ValueError('sample rates must be positive (got %d -> %d)' % (orig_freq, new_freq))
    g = math.gcd(orig_freq, new_freq)
    return orig_freq // g, new_freq // g


def _check_method(resampling_method, lowpass_filter_width):
    if resampling_method != 'sinc_interp_hann':
        raise ValueError("resampling_method %r is not implemented (only 'sinc_interp_hann', torchaudio's default)" % (resampling_method,))
    if lowpass_filter_width <= 0:
        raise ValueError('lowpass_filter_width must be positive')


@functools.lru_cache(maxsize=None)
def _sinc_resample_kernel(orig, new, lowpass_filter_width, rolloff):
    base = min(orig, new) * rolloff
    width = int(math.ceil(lowpass_filter_width * orig / base))
    idx = np.arange(-width, width + orig, dtype=np.float64) / orig                                   # [K]
    # torch forms the phase offsets as int64 / int, which is a float32 division; the float32 quotient is then promoted to float64 by
    # the addition.  The rounding is kept: it moves every tap of a phase by up to 3e-8 of a sample.
    phase = (np.arange(0, -new, -1).astype(np.float32) / np.float32(new)).astype(np.float64)
    t = phase[:, None] + idx[None, :]
    t = np.clip(t * base, -lowpass_filter_width, lowpass_filter_width)
    window = np.cos(t * math.pi / lowpass_filter_width / 2) ** 2
    t = t * math.pi
    with np.errstate(invalid='ignore', divide='ignore'):
        h = np.where(t == 0, 1.0, np.sin(t) / t)
    h = h * (window * (base / orig))
    h.setflags(write=False)
    return h, width, orig, new


def sinc_resample_kernel(orig_freq, new_freq, lowpass_filter_width=6, rolloff=0.99):
    """
    The polyphase tap table of the Hann-windowed sinc resampler: ``(taps, width, orig, new)`` with ``orig`` / ``new`` the rates
    divided by their gcd, ``taps`` float64 ``[new][K]``, ``K = 2 width + orig`` (read-only; cached per argument tuple).  Output
    ``q new + p`` is ``sum_k taps[p][k] x[q orig + k - width]``.  The device and ``resample_host`` use ``taps`` rounded to fp32.

    torchaudio's ``_get_sinc_resample_kernel`` for ``resampling_method='sinc_interp_hann'`` with ``dtype=None``, restated.
    PARITY UNPINNED: torchaudio is not installed here, the formula is written from its published source, not checked against it.
    """
    orig, new = _reduced(orig_freq, new_freq)
    _check_method('sinc_interp_hann', lowpass_filter_width)
    return _sinc_resample_kernel(orig, new, lowpass_filter_width, float(rolloff))


def _out_len(L, orig, new):
    return -(-new * L // orig)


def resample_host(waveform, orig_freq, new_freq, lowpass_filter_width=6, rolloff=0.99, resampling_method='sinc_interp_hann'):
    """
    ``resample`` on the CPU in float64: an ndarray or CPU tensor ``(..., L)`` -> a float64 CPU tensor ``(..., ceil(new L / orig))``.
    Written as torchaudio applies its kernel -- ``conv1d(pad(x, (width, width + orig)), taps, stride=orig)``, transposed, flattened,
    truncated -- with the float64 value of the fp32 taps, so that it differs from the device only by how the K products of an output
    are accumulated.
    """
    _check_method(resampling_method, lowpass_filter_width)
    x = (waveform.detach().cpu() if isinstance(waveform, torch.Tensor) else torch.from_numpy(np.array(waveform))).to(torch.float64)
    orig, new = _reduced(orig_freq, new_freq)
    if orig == new:
        return x
    taps, width, orig, new = sinc_resample_kernel(orig, new, lowpass_filter_width, rolloff)
    h = torch.from_numpy(taps.astype(np.float32).astype(np.float64))
    lead, L = x.shape[:-1], x.shape[-1]
    flat = x.reshape(-1, 1, L)
    padded = torch.nn.functional.pad(flat, (width, width + orig))
    y = torch.nn.functional.conv1d(padded, h[:, None, :], stride=orig)           # (B, new, floor(L / orig) + 1)
    y = y.transpose(1, 2).reshape(flat.shape[0], -1)[:, :_out_len(L, orig, new)]
    return y.reshape(lead + (y.shape[-1],))


# ---- the device route (csrc/resample.hip) ------------------------------------------------------------------------------------

RESAMPLE_TILE = 16             # frames (groups of `new` outputs) per workgroup of the general kernel (= tt_resample_tile())
RESAMPLE_DIRECT_TILE = 1024    # the same for the kernel of the small ratios, 2:1, 1:2, 3:2 (= tt_resample_direct_tile())
RESAMPLE_MAX_TAPS = 704        # K = 2 width + orig the kernels hold (= tt_resample_max_taps())
RESAMPLE_MAX_PHASES = 1024     # reduced new rate they accept (= tt_resample_max_phases())
_MAX_ROWS = 65535             # clips per launch (grid.y); more are served by further launches
_checked = False
_device_taps = {}


def _lib():
    global _checked
    lib = _hip.lib()
    if not _checked:
        built = (lib.tt_resample_tile(), lib.tt_resample_direct_tile(), lib.tt_resample_max_taps(), lib.tt_resample_max_phases())
        if built != (RESAMPLE_TILE, RESAMPLE_DIRECT_TILE, RESAMPLE_MAX_TAPS, RESAMPLE_MAX_PHASES):
            raise RuntimeError('libttrap_hip.so was built with resampler tiles / capacities %s, utils.audio says %s'
                               % (built, (RESAMPLE_TILE, RESAMPLE_DIRECT_TILE, RESAMPLE_MAX_TAPS, RESAMPLE_MAX_PHASES)))
        _checked = True
    return lib


def resample_tiles():
    """(tile, direct tile): frames per workgroup of the general kernel and of the small-ratio kernel, read from the library."""
    lib = _lib()
    return lib.tt_resample_tile(), lib.tt_resample_direct_tile()


def _plan(orig_freq, new_freq, lowpass_filter_width, rolloff, resampling_method):
    """(orig, new, width, K) after every check that needs no tensor; the capacities are checked here, before any launch."""
    _check_method(resampling_method, lowpass_filter_width)
    orig, new = _reduced(orig_freq, new_freq)
    if orig == new:
        return orig, new, 0, 0
    width = int(math.ceil(lowpass_filter_width * orig / (min(orig, new) * rolloff)))
    K = 2 * width + orig
    if K > RESAMPLE_MAX_TAPS or new > RESAMPLE_MAX_PHASES:
        raise ValueError('%d -> %d Hz needs %d taps per phase and %d phases; the kernels hold %d and %d (resample_host has no limit)'
                         % (orig_freq, new_freq, K, new, RESAMPLE_MAX_TAPS, RESAMPLE_MAX_PHASES))
    return orig, new, width, K


def _taps_on(device, orig, new, lowpass_filter_width, rolloff):
    """The fp32 tap table, transposed to [K][new] (the layout the kernels read), on ``device``; uploaded once per ratio and device."""
    key = (str(device), orig, new, lowpass_filter_width, float(rolloff))
    if key not in _device_taps:
        taps = sinc_resample_kernel(orig, new, lowpass_filter_width, rolloff)[0]
        _device_taps[key] = torch.from_numpy(np.ascontiguousarray(taps.astype(np.float32).T)).to(device)
    return _device_taps[key]


def _check_input(waveform, name):
    if not isinstance(waveform, torch.Tensor):
        raise RuntimeError('%s takes a GPU tensor (got %s); resample_host is the CPU function' % (name, type(waveform).__name__))
    _hip.require_cuda(waveform)
    if waveform.dtype == torch.float64:
        raise ValueError('%s takes fp32 / fp16 / bf16 tensors; float64 input is what the host function resample_host is for' % name)
    if waveform.dtype not in (torch.float32, torch.float16, torch.bfloat16):
        raise ValueError('unsupported dtype %s' % waveform.dtype)


def _launch(x, plan, lowpass_filter_width, rolloff, normalize):
    """x: (B, C, L) fp32 contiguous on the device, L >= 1 -> (B, Lout) fp32: mix + resample (+ inf-norm) on the current stream."""
    orig, new, width, _ = plan
    B, C, L = x.shape
    lib = _lib()
    Lout = _out_len(L, orig, new)
    y = torch.empty(B, Lout, dtype=torch.float32, device=x.device)
    n_part = lib.tt_resample_partials(L, orig, new)
    if n_part < 1:
        raise ValueError('tt_resample_partials refused L = %d at %d:%d' % (L, orig, new))
    partials = torch.empty(B, n_part, dtype=torch.float32, device=x.device) if normalize else None
    with torch.cuda.device(x.device):
        taps_t = _taps_on(x.device, orig, new, lowpass_filter_width, rolloff)
        st = _hip.stream_ptr()
        for b0 in range(0, B, _MAX_ROWS):                              # the clips ride on grid.y: at most 65535 per launch
            b1 = min(b0 + _MAX_ROWS, B)
            part = None if partials is None else partials[b0:b1]
            _hip.check(lib.tt_resample(_hip.ptr(x[b0:b1]), b1 - b0, C, L, _hip.ptr(taps_t), orig, new, width, _hip.ptr(y[b0:b1]), Lout,
                                       _hip.ptr(part), st), 'tt_resample')
            if normalize:
                _hip.check(lib.tt_resample_normalize(_hip.ptr(y[b0:b1]), b1 - b0, Lout, _hip.ptr(part), n_part, st), 'tt_resample_normalize')
    return y


def resample(waveform, orig_freq, new_freq, lowpass_filter_width=6, rolloff=0.99, resampling_method='sinc_interp_hann'):
    """
    ``torchaudio.functional.resample`` for device tensors ``(..., L)`` (reference ``AudioDataset.py:73``): returns
    ``(..., ceil(new L / orig))`` in the input's dtype, enqueued on the current stream without a host synchronisation.  fp16 / bf16
    inputs are upcast to fp32 and the result is cast back; ``orig_freq == new_freq`` returns the input unchanged; ``L == 0`` returns
    an empty tensor without a launch.  ``ValueError``: float64 input (use ``resample_host``), non-integer rates, a
    ``resampling_method`` other than ``'sinc_interp_hann'``, a ratio beyond the kernels' capacities (``RESAMPLE_MAX_TAPS`` taps per
    phase, ``RESAMPLE_MAX_PHASES`` phases).  CPU tensors raise ``RuntimeError``: there is no CPU fallback.
    """
    plan = _plan(orig_freq, new_freq, lowpass_filter_width, rolloff, resampling_method)
    _check_input(waveform, 'resample')
    if waveform.dim() < 1:
        raise ValueError('waveform must be (..., time)')
    orig, new = plan[:2]
    if orig == new:
        return waveform
    lead, L = waveform.shape[:-1], waveform.shape[-1]
    B = int(np.prod(lead, dtype=np.int64))
    if L == 0 or B == 0:
        return waveform.new_empty(lead + (_out_len(L, orig, new),))
    x = waveform.detach().reshape(B, 1, L).to(torch.float32).contiguous()
    y = _launch(x, plan, lowpass_filter_width, rolloff, normalize=False)
    return y.reshape(lead + (y.shape[-1],)).to(waveform.dtype)


def mix_resample(waveform, orig_freq, new_freq):
    """
    ``resample(torch.mean(waveform, dim=-2), orig_freq, new_freq)`` in one launch (reference ``AudioDataset.py:70-73``):
    ``(..., C, L)`` on the device (fp16 / bf16 upcast to fp32, the result cast back) -> ``(..., ceil(new L / orig))``.  The
    channels are added in index order in fp32 and divided by C as the samples are staged; C = 1 and C = 2 give the bits of the
    two-step form, C >= 3 its value to one rounding of the mean.
    """
    plan = _plan(orig_freq, new_freq, 6, 0.99, 'sinc_interp_hann')
    _check_input(waveform, 'mix_resample')
    if waveform.dim() < 2 or waveform.shape[-2] < 1 or waveform.shape[-1] < 1 or plan[0] == plan[1]:
        raise ValueError('mix_resample takes (..., C, L) with C, L >= 1 and two different rates')
    lead, (C, L) = waveform.shape[:-2], waveform.shape[-2:]
    if int(np.prod(lead, dtype=np.int64)) == 0:
        return waveform.new_empty(lead + (_out_len(L, plan[0], plan[1]),))
    y = _launch(waveform.detach().reshape(-1, C, L).to(torch.float32).contiguous(), plan, 6, 0.99, normalize=False)
    return y.reshape(lead + (y.shape[-1],)).to(waveform.dtype)


def prepare_audio(waveform, fs, sample_rate):
    """
    The three lines of ``AudioDataset.get_audio`` (reference ``AudioDataset.py:70-77``) for decoded audio that is already on the
    device: ``(C, N)`` -> ``(1, N')`` or a batch ``(B, C, N)`` -> ``(B, 1, N')``, ``N' = ceil(sample_rate N / fs)``.  Two launches:
    the channel mix fused into the resampler's load, with every workgroup leaving the peak of its outputs; then ``/= peak`` per row
    where the peak is non-zero.  An all-zero row stays zero; a NaN or inf sample does what ``r / r.abs().max()`` does in torch.
    With ``fs == sample_rate`` nothing is resampled: the mix is ``torch.mean`` and only the division is launched.
    """
    plan = _plan(fs, sample_rate, 6, 0.99, 'sinc_interp_hann')
    _check_input(waveform, 'prepare_audio')
    if waveform.dim() not in (2, 3):
        raise ValueError('prepare_audio takes (C, N) or (B, C, N) (got %s)' % (tuple(waveform.shape),))
    x = waveform.detach()
    x = (x[None] if x.dim() == 2 else x).to(torch.float32).contiguous()
    B, C, L = x.shape
    if C < 1:
        raise ValueError('prepare_audio needs at least one channel')
    orig, new = plan[:2]
    if L == 0 or B == 0:
        y = x.new_empty(B, _out_len(L, orig, new))
    elif orig == new:
        y = torch.mean(x, dim=1)                                      # a new tensor, also at C = 1
        peak = y.abs().amax(dim=1, keepdim=True)                      # one slot per row; amax carries a NaN like max
        with torch.cuda.device(x.device):
            for b0 in range(0, B, _MAX_ROWS):
                b1 = min(b0 + _MAX_ROWS, B)
                _hip.check(_lib().tt_resample_normalize(_hip.ptr(y[b0:b1]), b1 - b0, L, _hip.ptr(peak[b0:b1]), 1, _hip.stream_ptr()),
                           'tt_resample_normalize')
    else:
        y = _launch(x, plan, 6, 0.99, normalize=True)
    y = y.reshape(B, 1, -1).to(waveform.dtype)
    return y[0] if waveform.dim() == 2 else y
