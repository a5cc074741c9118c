"""
Drop-in for reference ``timbre_trap/framework/cqtwrapper.py`` (class ``CQT``): same constructor,
attributes (``sample_rate, hop_length, n_bins, midi_freqs, block_length, max_window_length``) and
methods, with the transform itself (``cqt_pytorch.CQT.encode/decode`` in the reference) computed by
the gfx950 kernels of csrc/cqt.hip through the C ABI ``tt_cqt_forward`` / ``tt_cqt_inverse``.

``encode``, ``analyze``, ``synthesize`` and ``magnitude`` take part in autograd, as the torch code the reference inherits from
``cqt_pytorch`` does: their backward is the other direction of the transform on the other window table (``tt_cqt_forward_bwd`` /
``tt_cqt_inverse_bwd`` / ``tt_cqt_forward_mag_bwd``; derivation in DESIGN.md 6j).  ``forward`` and ``decode`` stay detached: the
reference wraps exactly those two in ``torch.no_grad()`` (cqtwrapper.py:65, :199).

``griffin_lim`` and ``from_decibels`` are additions: the way from the magnitude variants' output back to audio (``tt_cqt_griffin_lim``,
DESIGN.md 6k), which the reference lacks.

The frame/time helpers (reference :215-308) stay pure Python/NumPy: the datasets call them from
DataLoader worker processes, so they must not touch the HIP runtime, and the object stays
fork- and pickle-safe (no library handle is stored on it).
"""

import ctypes
import math

import numpy as np
import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from .. import _hip
from . import nsgt_plan, ops

_TABLES = ('tw675', 'tw49', 'twNc', 'twN', 'tw1024', 'bin_tab', 'window', 'dual', 'gat_off', 'gat_idx')
_GENERIC_TABLES = ('chirp', 'bfilt', 'twP', 'twM', 'bin_tab', 'window', 'dual', 'gat_off', 'gat_idx', 'pos_bin')
# True: also the reference configuration (3 s @ 22.05 kHz) runs on the any-block-length kernels (csrc/cqt_generic.hip) -- for tests
# that hold the two paths against each other; read when a CQT is constructed
FORCE_GENERIC = False


def _aligned(t, nbytes):
    """``t`` (contiguous) at an address the kernels accept (include/ttrap.h: audio moves as pairs of samples, 8 bytes; interleaved complex
    coefficients 8): a contiguous view into a larger tensor may start anywhere, a copy starts on an allocation."""
    return t if t.data_ptr() % nbytes == 0 else t.clone()


def _wants_grad(t):
    return torch.is_grad_enabled() and t.requires_grad


# ---- autograd (kept here, not in ops: they bracket no bench event and take an unscaled gradient) --------------------------------------------
# fp32 inside autocast regions; the gradient is made contiguous fp32 / complex64 before the call (it commonly arrives through
# to_real's transposed view); no double backward.

class _AnalysisFn(torch.autograd.Function):
    """audio -> coefficients (CQT._transform); backward: tt_cqt_forward_bwd, the synthesis on the analysis windows times N / 2M."""

    @staticmethod
    @torch.amp.custom_fwd(device_type='cuda', cast_inputs=torch.float32)
    def forward(ctx, audio, cq, complex_out):
        ctx.cq, ctx.complex_out, ctx.shape, ctx.dtype = cq, complex_out, audio.shape, audio.dtype
        return cq._transform(audio, complex_out)

    @staticmethod
    @once_differentiable
    @torch.amp.custom_bwd(device_type='cuda')
    def backward(ctx, g):
        if not ctx.needs_input_grad[0]:
            return None, None, None
        cq = ctx.cq
        if ctx.complex_out:
            g = g.resolve_conj().to(torch.complex64).reshape(-1, 1, cq.n_bins, g.size(-1))
        else:
            g = g.to(torch.float32).reshape(-1, 2, cq.n_bins, g.size(-1))
        da = cq._synthesis(g, False, adjoint=True)
        return da.reshape(ctx.shape).to(ctx.dtype), None, None


class _SynthesisFn(torch.autograd.Function):
    """coefficients -> audio without the inf-norm (CQT._decode_raw); backward: tt_cqt_inverse_bwd, the analysis on the dual windows
    times 2M / N, in the layout the coefficients came in."""

    @staticmethod
    @torch.amp.custom_fwd(device_type='cuda', cast_inputs=torch.float32)
    def forward(ctx, coefficients, cq):
        ctx.cq, ctx.is_complex, ctx.shape, ctx.dtype = cq, coefficients.is_complex(), coefficients.shape, coefficients.dtype
        return cq._synthesis(coefficients, False)

    @staticmethod
    @once_differentiable
    @torch.amp.custom_bwd(device_type='cuda')
    def backward(ctx, g):
        if not ctx.needs_input_grad[0]:
            return None, None
        dc = ctx.cq._analysis(g.to(torch.float32).reshape(ctx.shape[0], -1), ctx.is_complex, adjoint=True)
        return dc.reshape(ctx.shape).to(ctx.dtype), None


class _MagnitudeFn(torch.autograd.Function):
    """audio -> |c| (tt_cqt_forward_mag); backward: tt_cqt_forward_mag_bwd on the saved audio -- the coefficients are recomputed in
    registers, neither they nor their gradient reach memory."""

    @staticmethod
    @torch.amp.custom_fwd(device_type='cuda', cast_inputs=torch.float32)
    def forward(ctx, audio, cq):
        ctx.cq, ctx.shape, ctx.dtype = cq, audio.shape, audio.dtype
        ctx.save_for_backward(audio)
        return cq._magnitude(audio)

    @staticmethod
    @once_differentiable
    @torch.amp.custom_bwd(device_type='cuda')
    def backward(ctx, g):
        if not ctx.needs_input_grad[0]:
            return None, None
        cq = ctx.cq
        audio, = ctx.saved_tensors
        a, _ = cq._prepare_audio(audio)
        B, n_blocks = a.size(0), a.size(1) // cq.block_length
        g = g.to(torch.float32).reshape(B, cq.n_bins, n_blocks * cq.max_window_length).contiguous()
        lib = _hip.lib()
        ps = cq._plan_struct(a.device)
        scratch = cq._scratch(lib, ps, B * n_blocks, a.device)
        da = torch.empty_like(a)
        with _hip.timed('cqt_forward_mag_bwd'):
            _hip.check(lib.tt_cqt_forward_mag_bwd(ctypes.byref(ps), _hip.ptr(a), _hip.ptr(g), _hip.ptr(da), _hip.ptr(scratch), B, n_blocks,
                                                  _hip.stream_ptr()), 'tt_cqt_forward_mag_bwd')
        return da.reshape(ctx.shape).to(ctx.dtype), None


class CQT(nn.Module):
    """
    Invertible constant-Q transform (NSGT, one block of ``secs_per_block`` seconds at a time).
    """

    def __init__(self, n_octaves, bins_per_octave, sample_rate, secs_per_block, conventions=None):
        """
        Parameters (reference cqtwrapper.py:15-29; ``conventions`` is an addition: an
        ``nsgt_plan.NSGTConventions`` selecting the window family / rounding / crop alignment / dual-window rule that the
        reference leaves to ``cqt_pytorch`` -- table-level switches, default documented in INTEGRATION.md)
        ----------
        n_octaves : int
          Number of octaves below Nyquist to span
        bins_per_octave : int
          Number of bins allocated to each octave
        sample_rate : int or float
          Number of samples per second of audio
        secs_per_block : float
          Number of seconds to process at a time
        """
        super().__init__()

        self.conventions = nsgt_plan.DEFAULT_CONVENTIONS if conventions is None else conventions
        plan = nsgt_plan.build_plan(n_octaves, bins_per_octave, sample_rate,
                                    int(secs_per_block * sample_rate), power_of_2_length=True, conventions=self.conventions,
                                    generic=FORCE_GENERIC)
        self.block_length = plan['N']
        self.max_window_length = plan['M']
        self._sum_len = plan['sum_len']
        # the reference configuration (N = 66150, M = 1024) runs on the specialised kernels of csrc/cqt.hip, every other block
        # length on the any-length path of csrc/cqt_generic.hip (same tables, same conventions; reference cqtwrapper.py:15-48
        # accepts any secs_per_block / sample_rate)
        self._fast = plan['fast']
        self._P = int(plan.get('P', 0))

        for name in (_TABLES if self._fast else _GENERIC_TABLES):
            a = plan[name]
            t = torch.from_numpy(np.ascontiguousarray(a)).to(torch.int32 if a.dtype.kind == 'i' else torch.float32)
            self.register_buffer('_t_' + name, t.contiguous(), persistent=False)

        self.sample_rate = sample_rate
        # reference cqtwrapper.py:40-48
        self.hop_length = (self.block_length / self.max_window_length)
        self.n_bins = n_octaves * bins_per_octave
        fmin = 12 * (np.log2(np.asanyarray((sample_rate / 2) / (2 ** n_octaves))) - np.log2(440.0)) + 69
        self.midi_freqs = fmin + np.arange(self.n_bins) / (bins_per_octave / 12)

    # ---- device side -------------------------------------------------------------------------

    def _plan_struct(self, device):
        if self._t_window.device != device:
            raise RuntimeError('CQT tables are on %s but the input is on %s; call .to(device) on the module'
                               % (self._t_window.device, device))
        ps = _hip.CqtPlan() if self._fast else _hip.CqtGenericPlan()
        for name in (_TABLES if self._fast else _GENERIC_TABLES):
            setattr(ps, name, getattr(self, '_t_' + name).data_ptr())
        ps.n_bins = self.n_bins
        ps.sum_len = self._sum_len
        if not self._fast:
            ps.N, ps.M, ps.P = self.block_length, self.max_window_length, self._P
        return ps

    def _scratch(self, lib, ps, n_clips, device):
        nbytes = (lib.tt_cqt_scratch_bytes(n_clips, self.n_bins, self._sum_len) if self._fast
                  else lib.tt_cqt_generic_scratch_bytes(ctypes.byref(ps), n_clips))
        if nbytes <= 0:
            raise RuntimeError('the constant-Q transform plan was rejected by the library (block_length=%d, max_window_length=%d)'
                               % (self.block_length, self.max_window_length))
        return torch.empty(nbytes, dtype=torch.uint8, device=device)

    def _prepare_audio(self, audio):
        _hip.require_cuda(audio)
        if audio.size(-1) % self.block_length:
            raise ValueError('audio length %d is not a multiple of the block length %d (use pad_to_block_length)'
                             % (audio.size(-1), self.block_length))
        lead = audio.shape[:-1]
        a = _aligned(audio.reshape(-1, audio.size(-1)).to(torch.float32).contiguous(), 8)
        return a, lead

    def _analysis(self, a, complex_out, adjoint=False):
        """a (B, n_blocks N) contiguous fp32 -> (B, 2, F, T) planes or complex (B, 1, F, T).  ``adjoint``: the gradient of the synthesis
        w.r.t. its coefficients instead (tt_cqt_inverse_bwd: the same pipeline on the dual windows, times 2M / N)."""
        a = _aligned(a.contiguous(), 8)
        B, n_blocks = a.size(0), a.size(1) // self.block_length
        T = n_blocks * self.max_window_length
        lib = _hip.lib()
        ps = self._plan_struct(a.device)
        scratch = self._scratch(lib, ps, B * n_blocks, a.device)
        if adjoint:
            entry, name = (lib.tt_cqt_inverse_bwd if self._fast else lib.tt_cqt_generic_inverse_bwd), 'cqt_inverse_bwd'
        else:
            entry, name = (lib.tt_cqt_forward if self._fast else lib.tt_cqt_generic_forward), 'cqt_forward'
        if complex_out:
            out = torch.empty((B, 1, self.n_bins, T, 2), dtype=torch.float32, device=a.device)
        else:
            out = torch.empty((B, 2, self.n_bins, T), dtype=torch.float32, device=a.device)
        with _hip.timed(name):
            _hip.check(entry(ctypes.byref(ps), _hip.ptr(a), _hip.ptr(out), _hip.ptr(scratch),
                             B, n_blocks, int(complex_out), _hip.stream_ptr()), 'tt_' + name)
        return torch.view_as_complex(out) if complex_out else out

    def _transform(self, audio, complex_out):
        a, lead = self._prepare_audio(audio)
        out = self._analysis(a, complex_out)
        # (B,1,N) input -> lead == (B,1): the channel dim of the reference output replaces it
        if len(lead) != 2:
            out = out.reshape(*lead, *out.shape[1:])
        return out

    def encode(self, audio):
        """audio (B x 1 x N) -> complex coefficients (B x 1 x F x T)   (cqtwrapper.py:67, sonify.py:94).  Differentiable w.r.t. the
        audio, as ``cqt_pytorch.CQT.encode`` is."""
        if _wants_grad(audio):
            return _AnalysisFn.apply(audio, self, True)
        with torch.no_grad():
            return self._transform(audio, True)

    def analyze(self, audio):
        """The values and layout of ``forward`` (B x 2 x F x T real/imaginary planes, contiguous), taking part in autograd: what
        ``to_real(encode(audio))`` is in the reference, without the transposed view."""
        if _wants_grad(audio):
            return _AnalysisFn.apply(audio, self, False)
        with torch.no_grad():
            return self._transform(audio, False)

    def synthesize(self, coefficients):
        """The raw synthesis ``cqt_pytorch.CQT.decode`` is (``super().decode`` at reference cqtwrapper.py:207): real (B x 2 x F x T) or
        complex (B x 1 x F x T) coefficients -> audio (B x 1 x T), no division by the infinity norm; differentiable w.r.t. the
        coefficients."""
        if _wants_grad(coefficients):
            return _SynthesisFn.apply(coefficients, self)
        return self._decode(coefficients, False)

    def forward(self, audio):
        """
        Encode a batch of audio into CQT spectral coefficients (reference cqtwrapper.py:50-72).

        audio : Tensor (B x 1 x T)  ->  coefficients : Tensor (B x 2 x F x T) real/imaginary
        """
        with torch.no_grad():
            return self._transform(audio, False)

    def magnitude(self, audio):
        """
        ``to_magnitude(forward(audio))`` in one pass: audio (B x 1 x N) -> magnitudes (B x F x T), the input of the magnitude variants
        (reference modules.py:948, :1019).  The reference configuration writes |c| from the transform's own epilogue
        (tt_cqt_forward_mag: the two coefficient planes never reach memory); other block lengths compose the any-length transform with
        tt_magnitude.  Differentiable w.r.t. the audio: tt_cqt_forward_mag_bwd on the saved audio, or (other block lengths) ``encode``
        composed with torch's norm.
        """
        if not self._fast:
            if _wants_grad(audio):
                return self.to_real(self.encode(audio)).norm(p=2, dim=-3)
            return self.to_magnitude(self.forward(audio))
        if _wants_grad(audio):
            return _MagnitudeFn.apply(audio, self)
        return self._magnitude(audio)

    def _magnitude(self, audio):
        with torch.no_grad():
            a, lead = self._prepare_audio(audio)
            B, n_blocks = a.size(0), a.size(1) // self.block_length
            lib = _hip.lib()
            ps = self._plan_struct(a.device)
            scratch = self._scratch(lib, ps, B * n_blocks, a.device)
            out = torch.empty((B, self.n_bins, n_blocks * self.max_window_length), dtype=torch.float32, device=a.device)
            with _hip.timed('cqt_forward_mag'):
                _hip.check(lib.tt_cqt_forward_mag(ctypes.byref(ps), _hip.ptr(a), _hip.ptr(out), _hip.ptr(scratch), B, n_blocks,
                                                  _hip.stream_ptr()), 'tt_cqt_forward_mag')
            # the shapes of to_magnitude(forward(audio)): (B,1,N) -> (B,F,T), any other lead -> (*lead, F, T)
            if len(lead) != 2:
                out = out.reshape(*lead, *out.shape[1:])
            return out

    def decode(self, coefficients):
        """
        Invert CQT spectral coefficients to synthesize audio (reference cqtwrapper.py:184-213).

        coefficients : Tensor (B x 2 OR 1 x F x T) real/imaginary OR complex -> audio (B x 1 x T),
        divided by its infinity norm when that is non-zero.
        """
        return self._decode(coefficients, True)

    def _decode_raw(self, coefficients):
        """The synthesis without the batch-wide division by the infinity norm (what ``cqt_pytorch.CQT.decode`` returns before
        reference cqtwrapper.py:209-211 rescales it); used by tests to compare clips of one batch independently."""
        return self._decode(coefficients, False)

    def _decode(self, coefficients, normalize):
        with torch.no_grad():
            return self._synthesis(coefficients, normalize)

    def _synthesis(self, coefficients, normalize, adjoint=False):
        """Coefficients (B, 2, F, T) or complex (B, 1, F, T) -> audio (B, 1, n_blocks N).  ``adjoint``: the gradient of the analysis
        w.r.t. its audio instead (tt_cqt_forward_bwd: the same pipeline on the analysis windows, times N / 2M, no inf-norm)."""
        _hip.require_cuda(coefficients)
        is_complex = coefficients.is_complex()
        if is_complex:
            c = torch.view_as_real(_aligned(coefficients.to(torch.complex64).contiguous(), 8))
            B = c.size(0)
            T = c.size(-2)
        else:
            c = coefficients.to(torch.float32).contiguous()
            B = c.size(0)
            T = c.size(-1)
        if T % self.max_window_length:
            raise ValueError('frame count %d is not a multiple of %d' % (T, self.max_window_length))
        n_blocks = T // self.max_window_length
        lib = _hip.lib()
        ps = self._plan_struct(c.device)
        scratch = self._scratch(lib, ps, B * n_blocks, c.device)
        audio = torch.empty((B, 1, n_blocks * self.block_length), dtype=torch.float32, device=c.device)
        if adjoint:
            entry = lib.tt_cqt_forward_bwd if self._fast else lib.tt_cqt_generic_forward_bwd
            with _hip.timed('cqt_forward_bwd'):
                _hip.check(entry(ctypes.byref(ps), _hip.ptr(c), _hip.ptr(audio), _hip.ptr(scratch),
                                 B, n_blocks, int(is_complex), _hip.stream_ptr()), 'tt_cqt_forward_bwd')
            return audio
        inverse = lib.tt_cqt_inverse if self._fast else lib.tt_cqt_generic_inverse
        with _hip.timed('cqt_inverse'):
            _hip.check(inverse(ctypes.byref(ps), _hip.ptr(c), _hip.ptr(audio), _hip.ptr(scratch),
                               B, n_blocks, int(is_complex), int(bool(normalize)), _hip.stream_ptr()), 'tt_cqt_inverse')
        return audio

    # ---- phase retrieval: audio from magnitudes (no reference counterpart; the magnitude variants' way to sonify.py) ----------------

    # True: the composed route (analysis with complex output, the projection as torch expressions, synthesis) also on the specialised
    # plan, where griffin_lim otherwise makes the one C call -- the yardstick of tests and of tools/kb_griffin_lim.py
    _gl_composed = False

    def griffin_lim(self, magnitude, n_iter=32, momentum=0.99, audio_init=None, normalize=True, return_convergence=False):
        """
        Audio whose transform has the given magnitudes, by the Griffin-Lim iteration with the momentum of "fast Griffin-Lim":

            c = analysis(x_k);  p = magnitude c / |c|  (magnitude + 0i where |c| == 0);  y_k = synthesis(p);
            x_{k+1} = y_k + momentum (y_k - y_{k-1}),  x_1 = y_0

        magnitude : fp32 Tensor (B x F x T) or (B x 1 x F x T) on the device, taken as given (no clamp)
        audio_init : Tensor (B x 1 x N) the start x_0, e.g. the mixture the magnitudes were estimated from; None = silence, which makes
          y_0 the zero-phase synthesis
        returns audio (B x 1 x N) = y_{n_iter-1}, divided by its infinity norm as ``decode`` does if ``normalize``; with
        ``return_convergence`` also the (n_iter x B) tensor of sqrt(sum (|c| - magnitude)^2 / sum magnitude^2) per clip, row k measured
        on the input x_k of iteration k.

        Always detached.  The reference configuration runs tt_cqt_griffin_lim: all iterations enqueued by one call, the coefficients
        never in memory.  Other block lengths (correct, untuned, as everywhere on the any-length path) loop here over the any-length
        analysis and synthesis with the projection, the convergence and the extrapolation as torch expressions.
        """
        _hip.require_cuda(magnitude, audio_init)
        if magnitude.dim() == 4 and magnitude.size(1) == 1:
            magnitude = magnitude[:, 0]
        if magnitude.dim() != 3 or magnitude.size(1) != self.n_bins:
            raise ValueError('magnitudes of shape %s, expected (B, %d, T) or (B, 1, %d, T)' % (tuple(magnitude.shape), self.n_bins, self.n_bins))
        B, T = magnitude.size(0), magnitude.size(2)
        if B == 0 or T == 0 or T % self.max_window_length:
            raise ValueError('frame count %d is not a positive multiple of %d' % (T, self.max_window_length))
        if int(n_iter) != n_iter or n_iter < 1:
            raise ValueError('n_iter = %r: at least one iteration' % (n_iter,))
        alpha = ctypes.c_float(momentum).value                      # the value the kernels see
        if not 0.0 <= alpha < 1.0:
            raise ValueError('momentum = %r is outside [0, 1)' % (momentum,))
        n_iter, n_blocks = int(n_iter), T // self.max_window_length
        with torch.no_grad():
            mag = magnitude.detach().to(torch.float32).contiguous()
            x = None
            if audio_init is not None:
                if audio_init.numel() != B * n_blocks * self.block_length or audio_init.size(0) != B:
                    raise ValueError('audio_init of shape %s for %d clips of %d blocks of %d samples'
                                     % (tuple(audio_init.shape), B, n_blocks, self.block_length))
                x = _aligned(audio_init.detach().reshape(B, -1).to(torch.float32).contiguous(), 8)
            if not self._fast or self._gl_composed:
                return self._griffin_lim_composed(mag, x, n_iter, alpha, normalize, return_convergence)
            lib = _hip.lib()
            ps = self._plan_struct(mag.device)
            nbytes = lib.tt_cqt_griffin_lim_scratch_bytes(B * n_blocks, self.n_bins, self._sum_len)
            if nbytes <= 0:
                raise RuntimeError('the constant-Q transform plan was rejected by the library')
            scratch = torch.empty(nbytes, dtype=torch.uint8, device=mag.device)
            audio = torch.empty((B, 1, n_blocks * self.block_length), dtype=torch.float32, device=mag.device)
            conv = torch.empty((n_iter, B), dtype=torch.float32, device=mag.device) if return_convergence else None
            with _hip.timed('cqt_griffin_lim'):
                _hip.check(lib.tt_cqt_griffin_lim(ctypes.byref(ps), _hip.ptr(mag), _hip.ptr(x), _hip.ptr(audio), _hip.ptr(conv),
                                                  _hip.ptr(scratch), B, n_blocks, n_iter, alpha, int(bool(normalize)), _hip.stream_ptr()),
                           'tt_cqt_griffin_lim')
            return (audio, conv) if return_convergence else audio

    def _griffin_lim_composed(self, mag, x, n_iter, alpha, normalize, return_convergence):
        """The same iteration on the two transforms' own entry points (on either plan): the coefficients and their projection pass
        through memory."""
        B = mag.size(0)
        m = mag[:, None]
        if x is None:
            x = torch.zeros((B, m.size(-1) // self.max_window_length * self.block_length), dtype=torch.float32, device=mag.device)
        conv, y_prev = [], None
        for k in range(n_iter):
            c = self._analysis(x, True)
            n = c.abs()
            if return_convergence:
                num, den = ((n - m).double() ** 2).sum((1, 2, 3)), (m.double() ** 2).sum((1, 2, 3))
                conv.append(torch.where(num == 0, torch.zeros_like(num), (num / den).sqrt()).float())
            p = torch.where(n == 0, torch.complex(m, torch.zeros_like(m)), c * (m / n))
            last = k == n_iter - 1
            audio = self._synthesis(p, normalize and last)
            if last:
                break
            y = audio.reshape(B, -1)
            x = y if y_prev is None or alpha == 0.0 else torch.add(y, y - y_prev, alpha=alpha)
            y_prev = y
        return (audio, torch.stack(conv)) if return_convergence else audio

    @staticmethod
    def from_decibels(decibels):
        """The inverse of ``to_decibels(rescale=True)`` up to each item's peak: 10^(4 (d - 1)), i.e. 1 at the item's maximum and 1e-4 on
        the 80 dB floor.  The scale that ``to_decibels`` removed is lost; the infinity norm of ``decode`` / ``griffin_lim`` removes it
        anyway."""
        return torch.pow(10.0, 4.0 * (decibels - 1.0))

    # ---- layout helpers (reference cqtwrapper.py:74-182), stock tensor views ----------------------

    @staticmethod
    def to_real(coefficients):
        """complex (B x 1 x F x T) -> real/imaginary (B x 2 x F x T)   (cqtwrapper.py:74-97)."""
        coefficients = coefficients.squeeze(-3)
        coefficients = torch.view_as_real(coefficients)
        return coefficients.transpose(-1, -2).transpose(-2, -3)

    @staticmethod
    def to_complex(coefficients):
        """real/imaginary (B x 2 x F x T) -> complex (B x F x T)   (cqtwrapper.py:99-120)."""
        coefficients = coefficients.transpose(-3, -2).transpose(-2, -1)
        return torch.view_as_complex(coefficients.contiguous())

    @staticmethod
    def _device_path(t):
        # fp32 GPU tensors outside autograd take the kernels; CPU tensors and inputs that require grad keep the torch expression
        return t.is_cuda and t.dtype == torch.float32 and not t.requires_grad

    @staticmethod
    def to_magnitude(coefficients):
        """L2 norm over the real/imaginary channel (cqtwrapper.py:122-141); GPU: tt_magnitude."""
        if CQT._device_path(coefficients) and coefficients.dim() >= 3 and coefficients.size(-3) == 2 and coefficients.numel() > 0:
            return ops.magnitude(coefficients)
        return coefficients.norm(p=2, dim=-3)

    @staticmethod
    def to_decibels(magnitude, rescale=True):
        """
        Amplitude -> dB per track with an 80 dB floor, optionally rescaled to [0, 1]
        (cqtwrapper.py:143-182; torchaudio AmplitudeToDB('amplitude', top_db=80) restated).  GPU: tt_decibels, the item maxima and the
        map in two launches for the whole batch.
        """
        if CQT._device_path(magnitude) and magnitude.dim() >= 1 and 0 < magnitude.size(0) <= 65535 and magnitude.numel() > 0:
            return ops.decibels(magnitude, rescale)
        decibels = list()
        for m in magnitude:
            d = 20.0 * torch.log10(torch.clamp(m, min=1e-10))
            d = torch.maximum(d, d.max() - 80.0)
            if rescale:
                d = d - d.max()
                d = 1 + d / 80
            decibels.append(d.unsqueeze(0))
        return torch.cat(decibels, dim=0)

    # ---- frame / time arithmetic (pure Python; reference cqtwrapper.py:215-308) -------------------

    def pad_to_block_length(self, audio):
        """Zero-pad to the next multiple of the block length (cqtwrapper.py:215-233)."""
        return torch.nn.functional.pad(audio, (0, -audio.size(-1) % self.block_length))

    def get_expected_samples(self, t):
        """Number of samples for ``t`` seconds, rounded down (cqtwrapper.py:235-253)."""
        return int(max(0, t) * self.sample_rate)

    def get_expected_frames(self, num_samples):
        """Number of frames returned for ``num_samples`` samples (cqtwrapper.py:255-273)."""
        return math.ceil((num_samples / self.block_length) * self.max_window_length)

    def get_times(self, n_frames):
        """Time in seconds of each frame (cqtwrapper.py:275-293)."""
        return np.arange(n_frames) * self.hop_length / self.sample_rate

    def get_midi_freqs(self):
        """Centre frequency (MIDI) of each bin (cqtwrapper.py:295-308)."""
        return self.midi_freqs

    # reference checkpoints carry cqt_pytorch buffers under sliCQ.*; ours are derived, so ignore them
    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys,
                              error_msgs):
        for k in [k for k in state_dict if k.startswith(prefix)]:
            state_dict.pop(k)
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys,
                                      error_msgs)
