"""
Drop-in for reference ``timbre_trap/framework/modules.py``: the Timbre-Trap autoencoder with the
reference's class names, constructor signatures, attribute names and ``state_dict`` keys, running on
the gfx950 kernels of libttrap_hip.so.

How it differs from the reference inside (the public behaviour does not):
  * ``nn.Conv2d`` / ``nn.ConvTranspose2d`` objects are kept only as PARAMETER CONTAINERS (so the
    keys, shapes and default initialisation are the reference's); their forward is never used.
    Each layer calls a hand-written kernel through ``ops`` (fused ResidualConv2dBlock, general
    direct convolution, latent GEMM) with a hand-written backward.
  * ``chunked_inference`` batches all 50 %-overlapping chunks through ONE encoder/decoder pass
    instead of a sequential Python loop (chunks are independent; the windowed overlap-add is
    unchanged and bit-identical in summation order).
"""

import os

import torch
import torch.nn as nn

from . import CQT
from . import ops
from .. import _hip
from .ops import ACT_ELU, ACT_NONE, ACT_RELU, ACT_SIGMOID, ConvCfg

__all__ = [
    'TimbreTrap',
    'Encoder',
    'Decoder',
    'EncoderBlock',
    'DecoderBlock',
    'ResidualConv2dBlock',
    'TimbreTrapFiLM',
    'FiLM',
    'TimbreTrapMag',
    'TimbreTrapMagDB'
]

# chunks of one chunked_inference call processed per batched pass (bounds activation memory)
MAX_CHUNK_BATCH = 96


def _level_channels(model_complexity, reverse=False):
    ch = tuple(round(c * 2 ** (model_complexity - 1)) for c in (2, 4, 8, 16, 32))
    return ch[::-1] if reverse else ch


class ResidualConv2dBlock(nn.Module):
    """
    y = ELU(conv1x1(ELU(conv_kxk_dilated(x)))) + x with 'same' padding (reference modules.py:721-777).
    One fused kernel forward, one fused backward (csrc/conv_mfma.hip, csrc/conv_small.hip).
    """

    def __init__(self, in_channels, out_channels, kernel_size=3, dilation=1):
        nn.Module.__init__(self)
        self.conv1 = nn.Sequential(
            nn.Conv2d(in_channels, out_channels, kernel_size=kernel_size, padding='same', dilation=dilation),
            nn.ELU(inplace=True))
        self.conv2 = nn.Sequential(nn.Conv2d(out_channels, out_channels, kernel_size=1), nn.ELU(inplace=True))
        self.dilation = dilation

    def forward(self, x):
        c1, c2 = self.conv1[0], self.conv2[0]
        return ops.residual_block(x, c1.weight, c1.bias, c2.weight, c2.bias, self.dilation)


class EncoderBlock(nn.Module):
    """
    Three residual blocks (dilation 1, 2, 3) then a (2*stride, 1) convolution with stride
    (stride, 1) + ELU that halves the frequency axis (reference modules.py:597-655).
    """

    def __init__(self, in_channels, out_channels, stride=2):
        nn.Module.__init__(self)
        self.block1 = ResidualConv2dBlock(in_channels, in_channels, kernel_size=3, dilation=1)
        self.block2 = ResidualConv2dBlock(in_channels, in_channels, kernel_size=3, dilation=2)
        self.block3 = ResidualConv2dBlock(in_channels, in_channels, kernel_size=3, dilation=3)
        self.hop = stride
        self.win = 2 * stride
        self.sconv = nn.Sequential(
            nn.Conv2d(in_channels, out_channels, kernel_size=(self.win, 1), stride=(self.hop, 1)),
            nn.ELU(inplace=True))

    def forward(self, x, out_x3=False, link_in=None, link_out=None):
        """out_x3 (inside ops.x3_chain_scope only): the caller's next layer takes a split-operand tensor.  link_in / link_out
        (Encoder.forward): ops.GateLink with the strided layer in front of this block's level / between this block's strided layer and
        the next block's level."""
        y = ops.residual_level(x, (self.block1, self.block2, self.block3), out_x3=ops.x3_chain(), link=link_in)
        s = self.sconv[0]
        return ops.strided_conv(y, s.weight, s.bias, self.win, self.hop, out_x3=out_x3, link=link_out)


class DecoderBlock(nn.Module):
    """
    (2*stride, 1) transposed convolution with stride (stride, 1) and output padding + ELU, then
    three residual blocks (reference modules.py:658-718).
    """

    def __init__(self, in_channels, out_channels, stride=2, padding=0):
        nn.Module.__init__(self)
        self.hop = stride
        self.win = 2 * stride
        self.out_pad = padding
        self.tconv = nn.Sequential(
            nn.ConvTranspose2d(in_channels, out_channels, kernel_size=(self.win, 1), stride=(self.hop, 1),
                               output_padding=(padding, 0)),
            nn.ELU(inplace=True))
        self.block1 = ResidualConv2dBlock(out_channels, out_channels, kernel_size=3, dilation=1)
        self.block2 = ResidualConv2dBlock(out_channels, out_channels, kernel_size=3, dilation=2)
        self.block3 = ResidualConv2dBlock(out_channels, out_channels, kernel_size=3, dilation=3)

    def forward(self, x, out_x3=False, uplink=None, join=None):
        """``join`` (ops.SkipJoin): the skip connection behind this block (reference modules.py:569-589 `y = block(y) + skip`), applied here so
        that the level's last kernel can take it in its epilogue."""
        t = self.tconv[0]
        # y has no consumer but the level: the level's backward may hand the transposed layer its gradient already gated (ops.GateLink)
        link = ops.gate_link() if torch.is_grad_enabled() else None
        y = ops.transposed_conv(x, t.weight, t.bias, self.win, self.hop, self.out_pad, out_x3=ops.x3_chain(), link=link, uplink=uplink)
        return ops.residual_level(y, (self.block1, self.block2, self.block3), out_x3=out_x3, link=link, join=join)


class EmbeddingList(list):
    """The encoder's five embeddings as the reference returns them (a list of tensors: modules.py:470-483), plus what the fused skip joins
    of the 16-bit path need (ops.SkipJoin): ``raw[i]`` -- the layer's own output tensor where ``self[i]`` is its gate tap (ops.gate_tap) --
    and ``links[i]``, the ops.GateLink of that layer (None without one)."""

    def __init__(self, tensors, raw, links):
        list.__init__(self, tensors)
        self.raw, self.links = list(raw), list(links)


class Encoder(nn.Module):
    """2-D convolutional encoder: coefficients (B,2,F,T) -> latents (B,D,T) (reference modules.py:396-483)."""

    def __init__(self, feature_size, latent_size=None, model_complexity=1):
        nn.Module.__init__(self)
        channels = _level_channels(model_complexity)
        if latent_size is None:
            latent_size = 32 * 2 ** (model_complexity - 1)

        self.convin = nn.Sequential(nn.Conv2d(2, channels[0], kernel_size=3, padding='same'), nn.ELU(inplace=True))
        self.block1 = EncoderBlock(channels[0], channels[1], stride=2)
        self.block2 = EncoderBlock(channels[1], channels[2], stride=2)
        self.block3 = EncoderBlock(channels[2], channels[3], stride=2)
        self.block4 = EncoderBlock(channels[3], channels[4], stride=2)

        embedding_size = feature_size
        for _ in range(4):
            embedding_size = embedding_size // 2 - 1
        self.convlat = nn.Conv2d(channels[4], latent_size, kernel_size=(embedding_size, 1))

    def forward(self, coefficients):
        """returns (latents (B,D,T), [5 embeddings], {})."""
        c = self.convin[0]
        blocks = (self.block1, self.block2, self.block3, self.block4)
        # the output of a block's strided layer is the next block's level input AND an embedding handed to the caller: the level's backward
        # hands the strided layer its gradient already gated (ops.GateLink), the caller's copy goes through ops.gate_tap
        # (the first one: between convin and the first level; the last one: between the last strided layer and the latent head)
        links = [ops.gate_link() if torch.is_grad_enabled() else None for _ in range(len(blocks) + 1)]
        raw = ops.conv(coefficients, c.weight, c.bias, ConvCfg(3, 3, 1, 1, 1, 1, 'conv', 0, ACT_ELU), link=links[0])
        embeddings, raws = [ops.gate_tap(raw, links[0])], [raw]
        for i, block in enumerate(blocks):
            # inside ops.x3_chain_scope (embeddings dropped by the caller): a block whose successor starts with a split-operand level
            # hands its output over in that layout
            if i + 1 < len(blocks):
                takes_x3 = blocks[i + 1].block1.conv1[0].in_channels in ops.X3_CHANNELS
            else:                                                # the latent head
                takes_x3 = ops.x3_latent_ok(block.sconv[0].out_channels, self.convlat.out_channels, w_enc=self.convlat.weight)
            raw = block(raw, out_x3=ops.x3_chain() and takes_x3, link_in=links[i], link_out=links[i + 1])
            embeddings.append(ops.gate_tap(raw, links[i + 1]))
            raws.append(raw)
        top = raw
        E = top.size(1) if ops.is_x3(top) else top.size(-2)
        if E != self.convlat.kernel_size[0]:
            raise ValueError('feature size %d does not match the latent head (%d)' % (E, self.convlat.kernel_size[0]))
        latents = ops.latent_encode(top, self.convlat.weight, self.convlat.bias, link=links[-1])
        return latents, EmbeddingList(embeddings, raws, links), dict()


class Decoder(nn.Module):
    """2-D convolutional decoder: latents (B,D+1,T) -> logits (B,2,F,T) (reference modules.py:486-594)."""

    def __init__(self, feature_size, latent_size=None, model_complexity=1):
        nn.Module.__init__(self)
        channels = _level_channels(model_complexity, reverse=True)
        if latent_size is None:
            latent_size = 32 * 2 ** (model_complexity - 1)

        padding = list()
        embedding_size = feature_size
        for _ in range(4):
            padding.append(embedding_size % 2)
            embedding_size = embedding_size // 2 - 1
        padding.reverse()

        self.convin = nn.Sequential(
            nn.ConvTranspose2d(latent_size + 1, channels[0], kernel_size=(embedding_size, 1)),
            nn.ELU(inplace=True))
        self.block1 = DecoderBlock(channels[0], channels[1], stride=2, padding=padding[0])
        self.block2 = DecoderBlock(channels[1], channels[2], stride=2, padding=padding[1])
        self.block3 = DecoderBlock(channels[2], channels[3], stride=2, padding=padding[2])
        self.block4 = DecoderBlock(channels[3], channels[4], stride=2, padding=padding[3])
        self.convout = nn.Conv2d(channels[4], 2, kernel_size=3, padding='same')

    def forward(self, latents, encoder_embeddings=None, indicator=None, pair=False, act=ACT_NONE):
        """``indicator``: None (latents carry the switch channel, the reference's call) or its constant value (then latents have
        one channel less and ops.latent_decode supplies it), or with ``pair`` the values of the two halves, which are then both decoded
        from the one batch of latents.  ``pair`` (TimbreTrap.decode_pair): the batch is two batches back to
        back; returns their two logits tensors.  ``encoder_embeddings``: the scaled embeddings (reference modules.py:569-589) or
        ops.SkipJoin descriptors (TimbreTrap.skip_joins: weight and join in one pass; with ``pair`` each serves both halves).
        ``act``: a nonlinearity behind convout, applied in its epilogue (the magnitude variants' decode: TimbreTrap.OUT_ACT)."""
        c = self.convin[0]
        skips = None if encoder_embeddings is None else list(encoder_embeddings)[::-1]
        # (inside ops.x3_chain_scope, no skip connections: the head hands a split-operand tensor to block1's transposed layer)
        # without skip connections the head's output goes straight (and only) into block1's transposed layer: that layer's backward may
        # hand the head its gradient already gated (ops.GateLink)
        uplink = ops.gate_link() if (skips is None and torch.is_grad_enabled()) else None
        y = ops.latent_decode(latents, c.weight, c.bias, indicator,
                              out_x3=skips is None and ops.x3_chain() and self.block1.tconv[0].out_channels in ops.X3_CHANNELS, link=uplink)
        if skips is not None:
            y = ops.skip_join(y, skips[0])
        blocks = (self.block1, self.block2, self.block3, self.block4)
        for i, block in enumerate(blocks):
            # transposed layers with a split-operand kernel: 64 -> 32 and 32 -> 16 channels (tt_x3_tconv_fwd)
            t = blocks[i + 1].tconv[0] if i + 1 < len(blocks) else None
            fold = skips is not None and isinstance(skips[i + 1], ops.SkipJoin)
            y = block(y, out_x3=skips is None and ops.x3_chain() and t is not None and (t.in_channels, t.out_channels) in ((64, 32), (32, 16)),
                      uplink=uplink if i == 0 else None, join=skips[i + 1] if fold else None)
            if skips is not None and not fold:
                y = ops.skip_join(y, skips[i + 1])
        o = self.convout
        if pair:
            return ops.conv_out_pair(y, o.weight, o.bias, act)
        return ops.conv(y, o.weight, o.bias, ConvCfg(3, 3, 1, 1, 1, 1, 'conv', 0, act))


class TimbreTrap(nn.Module):
    """
    CQT + encoder + switchable decoder (reference modules.py:23-393).  Attribute names
    (``sliCQ``, ``encoder``, ``decoder``, ``skip_weights``) follow the reference because every
    script of the reference reaches into them.
    """

    PAIR_DECODE = os.environ.get('TTRAP_PAIR_DECODE', '1') != '0'
    # the nonlinearity every decoder output goes through (decode, decode_pair): none here, relu / sigmoid in the magnitude variants
    OUT_ACT = ACT_NONE

    def __init__(self, sample_rate, n_octaves, bins_per_octave, secs_per_block=3,
                 latent_size=None, model_complexity=1, skip_connections=False):
        nn.Module.__init__(self)
        self.sliCQ = CQT(n_octaves=n_octaves, bins_per_octave=bins_per_octave,
                         sample_rate=sample_rate, secs_per_block=secs_per_block)
        self.encoder = Encoder(feature_size=self.sliCQ.n_bins, latent_size=latent_size, model_complexity=model_complexity)
        self.decoder = Decoder(feature_size=self.sliCQ.n_bins, latent_size=latent_size, model_complexity=model_complexity)
        self.skip_weights = torch.nn.Parameter(torch.ones(5)) if skip_connections else None

    def encode(self, audio):
        """audio (B,1,N) -> (latents (B,D,T), embeddings, {})."""
        return self.encoder(self.sliCQ(audio))

    def apply_skip_connections(self, embeddings):
        """Scale each encoder embedding by its learnable weight, or drop them (no skip connections)."""
        if self.skip_weights is None:
            return None
        return [ops.scale(e, self.skip_weights, i) for i, e in enumerate(embeddings)]

    def skip_joins(self, embeddings, defer=False):
        """What ``forward`` hands the decoder instead of ``apply_skip_connections(embeddings)`` on the 16-bit channels-last path: one
        ops.SkipJoin per embedding -- ``skip_weights[i] * e_i`` and the decoder's ``y + skip`` (reference modules.py:112, :569-589) are
        then ONE pass each way, on the encoder's own output tensors.  None where that does not apply (no skip connections, fp32 path,
        embeddings that did not come from this encoder as 16-bit tensors, ops.SKIP_FUSED off).
        ``defer`` (what ``forward`` passes): the embedding's share of a join's backward may be left to the backward of the encoder layer
        behind the embedding (ops._join_backward) -- valid only where the decoder also takes the LATENTS of the same encoder pass, so that
        every encoder layer's backward is certain to run after the joins': with detached latents those layers would never be reached and
        the parked gradients would be lost.  Callers composing encode / decode themselves keep the default."""
        if (self.skip_weights is None or not ops.SKIP_FUSED or not ops.cl16_mode() or not isinstance(embeddings, EmbeddingList)
                or not all(ops.is_cl16(e) and e.numel() % 8 == 0 for e in embeddings.raw)):
            return None
        return [ops.SkipJoin(e, self.skip_weights, i, link, defer) for i, (e, link) in enumerate(zip(embeddings.raw, embeddings.links))]

    def decode(self, latents, embeddings=None, transcribe=False):
        """latents (B,D,T) -> logits (B,2,F,T); the extra latent channel is 1 for reconstruction, 0 for transcription."""
        value = 0.0 if transcribe else 1.0
        if ops.cl16_mode():
            # the 16-bit latent head takes the indicator as a constant channel: no concatenated copy of the latents, and their
            # gradient comes back contiguous
            return self.decoder(latents, embeddings, indicator=value, act=self.OUT_ACT)
        indicator = torch.full_like(latents[..., :1, :], value)
        return self.decoder(torch.cat((latents, indicator), dim=-2), embeddings, act=self.OUT_ACT)

    def decode_pair(self, latents, embeddings=None):
        """(decode(latents, embeddings), decode(latents, embeddings, True)) -- the reconstruction and the transcription of the same
        latents (reference modules.py:365-371 calls decode twice).  On the 16-bit training path the two are ONE pass of the decoder
        over a batch of 2 B (clips are independent: the same values; half the launches, weight-gradient reduces and kernel tails of
        the decoder) -- without skip connections, or with them as ops.SkipJoin descriptors (``skip_joins``: each embedding then serves
        both halves, round 6); already scaled embedding TENSORS would have to be duplicated: two passes.
        TTRAP_PAIR_DECODE=0 / TimbreTrap.PAIR_DECODE = False: two passes."""
        joins = embeddings is not None and all(isinstance(e, ops.SkipJoin) and ops.is_cl16(e.e) for e in embeddings)
        if self.PAIR_DECODE and (embeddings is None or joins) and ops.cl16_mode() and torch.is_grad_enabled() and latents.dim() == 3:
            # the latents as they are: the 16-bit latent head expands both halves from them, each with its indicator as a constant channel,
            # and its backward returns the sum of the halves' gradients (ops.LatDec16Fn ``pair``) -- no concatenated copies
            return self.decoder(latents, embeddings, indicator=(1.0, 0.0), pair=True, act=self.OUT_ACT)
        return self.decode(latents, embeddings), self.decode(latents, embeddings, True)

    def _inference(self, audio, transcribe=False, check=True):
        # without skip connections the embeddings are dropped right here: the layers may keep their activations in the split-operand
        # layout between two wide levels (ops.x3_chain_scope; fp32 semantics, no autocast, no grad)
        with torch.no_grad():
            took_x3 = ops.x3_inference()
            with ops.x3_chain_scope(self.skip_weights is None), ops.x3_vouched_scope():
                latents, embeddings, _ = self.encode(audio)
                out = self.decode(latents, self.apply_skip_connections(embeddings), transcribe)
            # check=False: the caller checks what it makes of the chunks once (chunked_inference)
            if check and took_x3 and not ops.x3_vouched() and not ops.x3_range_ok(out):
                # an activation or weight beyond the split representation's range (|v| > 65504) comes out of csrc/conv_x3.hip
                # non-finite: the reference's fp32 evaluation stays finite there -- repeat on the fp32 kernels (ops.x3_range_ok)
                with ops.x3_disabled():
                    latents, embeddings, _ = self.encode(audio)
                    out = self.decode(latents, self.apply_skip_connections(embeddings), transcribe)
            return out

    def inference(self, audio, transcribe=False):
        """Full-length inference after zero-padding to a whole number of blocks."""
        return self._inference(self.sliCQ.pad_to_block_length(audio), transcribe)

    def chunked_inference(self, audio, transcribe=False):
        """
        Inference over 50 %-overlapping blocks with a (symmetric) Hann cross-fade
        (reference modules.py:204-269).  All chunks go through the network as one batch.  The range check of the split-operand
        kernels (ops.x3_range_ok: one reduction + one host sync) is made ONCE, on the cross-faded result, not per pass.
        """
        took_x3 = ops.x3_inference() and not ops.x3_vouched()
        coefficients = self._chunked(audio, transcribe)
        if took_x3 and not ops.x3_range_ok(coefficients):
            with ops.x3_disabled():               # beyond the split format's range somewhere: the fp32 kernels, like the reference
                coefficients = self._chunked(audio, transcribe)
        return coefficients

    def _chunked(self, audio, transcribe):
        B, F = audio.size(0), self.sliCQ.n_bins
        K = self.decoder.convout.out_channels              # channels of a chunk's output: 2, or 1 in the magnitude variants
        block, M = self.sliCQ.block_length, self.sliCQ.max_window_length
        audio = self.sliCQ.pad_to_block_length(audio)
        hop = block // 2
        audio = torch.nn.functional.pad(audio, [hop] * 2)
        n_chunks = (audio.size(-1) - hop) // hop
        window = torch.signal.windows.hann(M, dtype=torch.float32, device=audio.device)
        n_frames = self.sliCQ.get_expected_frames(audio.size(-1))
        coefficients = torch.zeros((B, K, F, n_frames), dtype=torch.float32, device=audio.device)

        # (B,1,n_chunks,block) view of the overlapping chunks
        chunks = audio.unfold(-1, block, hop)
        assert chunks.size(-2) == n_chunks
        per_pass = max(1, MAX_CHUNK_BATCH // B)
        lib = _hip.lib()
        for c0 in range(0, n_chunks, per_pass):
            c1 = min(n_chunks, c0 + per_pass)
            batch = chunks[:, :, c0:c1].permute(2, 0, 1, 3).reshape((c1 - c0) * B, 1, block)
            out = self._inference(batch, transcribe, check=False)     # ((c1 - c0) * B, K, F, M), chunk-major
            out = out.float().contiguous()                            # the kernel reads contiguous fp32 chunks (a no-op for the stock decoder)
            if out.shape != ((c1 - c0) * B, K, F, M):
                raise RuntimeError('chunk outputs of shape %s, expected %s' % (tuple(out.shape), ((c1 - c0) * B, K, F, M)))
            # out[b, :, :, i*M/2 : i*M/2 + M] += window * chunk_i, ascending i: the reference's accumulation order (tt_window_ola)
            if M % 8 == 0 and n_frames % 4 == 0:
                _hip.check(lib.tt_window_ola(_hip.ptr(out), _hip.ptr(window), _hip.ptr(coefficients), B * K * F, M, c0, c1, n_frames,
                                             _hip.stream_ptr()), 'tt_window_ola')
            else:       # frame counts the kernel's 16-byte accesses do not cover: the same sums as strided adds, same order
                out = out.view(c1 - c0, B, K, F, M)
                for i in range(c0, c1):
                    coefficients[..., i * (M // 2): i * (M // 2) + M] += window * out[i - c0]
        coefficients = coefficients[..., M // 2: -M // 2]
        if K == 1:
            # the reference adds the (B,1,F,M) chunk outputs into a zeros((B,2,F,T)) buffer (modules.py:240-263): broadcasting leaves two
            # equal channels, and transcribe / reconstruct see that (B,2,F,T) tensor
            coefficients = torch.cat((coefficients, coefficients), dim=1)
        return coefficients

    def to_activations(self, coefficients):
        """logits (B,2,F,T) -> activations (B,F,T) in [0,1): tanh of the complex magnitude."""
        return ops.ActivationsFn.apply(coefficients)

    def transcribe(self, audio):
        """audio (B,1,N) -> multi-pitch activations (B,F,T)."""
        return self.to_activations(self.chunked_inference(audio, True))

    def transcribe_notes(self, audio, **kwargs):
        """audio (B,1,N) -> note events (utils.events.NoteEvents: item, row, onset, end, n_active, peak, pitch) formed on the device from
        ``transcribe(audio)``; ``kwargs`` as for ``utils.note_events`` (t, peaks_only, n_valid_bins, resolution, max_gap, min_frames, order)."""
        from ..utils.events import note_events
        return note_events(self.transcribe(audio), self.sliCQ.midi_freqs, **kwargs)

    def transcribe_contours(self, audio, units_per_semitone=4096, **kwargs):
        """audio (B,1,N) -> ``(NoteEvents, NoteContours)``: the notes of ``transcribe_notes(audio, **kwargs)`` and, from the same one run of
        ``transcribe``, the per-frame pitch contour and pitch bends of every note (utils.contours.note_contours, formed on the device with
        the grouping and threshold arguments of ``kwargs``)."""
        from ..utils.contours import note_contours
        from ..utils.events import note_events
        activations, midi_freqs = self.transcribe(audio), self.sliCQ.midi_freqs
        events = note_events(activations, midi_freqs, **kwargs)
        shared = {k: kwargs[k] for k in ('t', 'peaks_only', 'n_valid_bins', 'resolution', 'bin_groups') if k in kwargs}
        return events, note_contours(activations, events, midi_freqs, units_per_semitone=units_per_semitone, **shared)

    def reconstruct(self, audio_in):
        """audio (B,1,N) -> re-synthesised audio (B,1,L)."""
        return self.sliCQ.decode(self.chunked_inference(audio_in, False))

    def sonify(self, coefficients):
        """coefficients (B,2,F,T) or complex (B,1,F,T) -> audio (B,1,N): what experiments/sonify.py:109 does with the model's output.
        The magnitude variants override it, so that loop runs on any variant with this one call."""
        return self.sliCQ.decode(coefficients)

    def forward(self, audio, consistency=False):
        """
        One pass for training / evaluation (reference modules.py:338-393): returns
        (reconstruction, latents, transcription, transcription_rec, transcription_scr, losses).
        """
        latents, embeddings, losses = self.encode(audio)
        # (defer: encoder and decoder are one graph here, so the joins' backward may be folded into the encoder layers' -- ops._join_backward)
        embeddings = self.skip_joins(embeddings, defer=True) or self.apply_skip_connections(embeddings)
        reconstruction, transcription = self.decode_pair(latents, embeddings)
        transcription_rec = transcription_scr = None
        if consistency:
            latents_trn, embeddings_trn, _ = self.encoder(transcription)
            embeddings_trn = self.skip_joins(embeddings_trn, defer=True) or self.apply_skip_connections(embeddings_trn)
            transcription_rec, transcription_scr = self.decode_pair(latents_trn, embeddings_trn)
        return reconstruction, latents, transcription, transcription_rec, transcription_scr, losses


class TimbreTrapFiLM(TimbreTrap):
    """
    FiLM variant (reference modules.py:780-844): the decoder is switched between reconstruction and transcription by a per-channel affine
    map of the latents, y = x * gamma(c) + beta(c) with c = (transcribe, not transcribe), instead of a constant extra latent channel;
    ``Decoder.convin`` takes ``latent_size`` channels.  The map is one streaming kernel each way (csrc/film.hip, ops.FilmFn) on the fp32
    latents of every route; everything behind it -- latent head, levels, skip joins, pair decode over 2 B clips -- is TimbreTrap's.
    ``latent_size`` must be given: the reference itself cannot construct this model without one (modules.py:799 reads ``in_channels`` of
    an nn.Sequential), so no checkpoint of such a model exists.
    """

    def __init__(self, sample_rate, n_octaves, bins_per_octave, secs_per_block=3,
                 latent_size=None, model_complexity=1, skip_connections=False):
        if latent_size is None:
            raise NotImplementedError('TimbreTrapFiLM needs an explicit latent_size: with latent_size=None the reference raises while it '
                                      'constructs the model (modules.py:799), so there is nothing to be compatible with')
        TimbreTrap.__init__(self, sample_rate, n_octaves, bins_per_octave, secs_per_block,
                            latent_size, model_complexity, skip_connections)
        # in the reference's order (the default initialisation draws from the RNG in this order)
        convin_out_channels = self.decoder.convin[0].out_channels
        convin_kernel_size = self.decoder.convin[0].kernel_size
        self.decoder.convin = nn.Sequential(
            nn.ConvTranspose2d(latent_size, convin_out_channels, kernel_size=convin_kernel_size),
            nn.ELU(inplace=True))
        self.film_layer = FiLM(latent_size, n_conditions=2)

    def decode(self, latents, embeddings=None, transcribe=False):
        """latents (B,D,T) -> logits (B,2,F,T); the condition is the one-hot pair (transcribe, not transcribe)."""
        z = self.film_layer(latents, (float(bool(transcribe)), float(not transcribe)))
        return self.decoder(z, embeddings, indicator=None, act=self.OUT_ACT)

    def decode_pair(self, latents, embeddings=None):
        """(decode(latents, embeddings), decode(latents, embeddings, True)).  Where TimbreTrap.decode_pair runs the decoder once over 2 B
        clips, so does this: the pair form of the FiLM kernel reads the latents once and writes the modulated reconstruction half and
        transcription half back to back -- no concatenated copies."""
        joins = embeddings is not None and all(isinstance(e, ops.SkipJoin) and ops.is_cl16(e.e) for e in embeddings)
        if self.PAIR_DECODE and (embeddings is None or joins) and ops.cl16_mode() and torch.is_grad_enabled() and latents.dim() == 3:
            f = self.film_layer
            z2 = ops.film_modulate(latents, f.gamma.weight, f.gamma.bias, f.beta.weight, f.beta.bias, (0.0, 1.0, 1.0, 0.0), reps=2)
            return self.decoder(z2, embeddings, indicator=None, pair=True, act=self.OUT_ACT)
        return self.decode(latents, embeddings), self.decode(latents, embeddings, True)


class TimbreTrapMag(TimbreTrap):
    """
    Magnitude-CQT (amplitude) variant (reference modules.py:892-997): the encoder takes |c| as ONE channel, the decoder returns one
    channel through a relu.  The interior -- levels, strided and transposed layers, latent heads, skip joins -- is TimbreTrap's.
      * encode:          CQT.magnitude (the transform writes |c| from its epilogue) -> (B,1,F,T)
      * decode:          relu fused into Decoder.convout's epilogue (tt_conv2d TT_ACT_RELU), on every route incl. decode_pair
      * to_activations:  tanh of the squeezed logits (tt_activations1_fwd)
      * chunked_inference / transcribe / reconstruct: the 1-channel chunks are cross-faded as one channel and returned as the
        reference's two equal channels (TimbreTrap._chunked)
    """

    OUT_ACT = ACT_RELU

    def __init__(self, sample_rate, n_octaves, bins_per_octave, secs_per_block=3,
                 latent_size=None, model_complexity=1, skip_connections=False):
        TimbreTrap.__init__(self, sample_rate, n_octaves, bins_per_octave, secs_per_block,
                            latent_size, model_complexity, skip_connections)
        # in the reference's order (the default initialisation draws from the RNG in this order)
        convin_out_channels = self.encoder.convin[0].out_channels
        convout_in_channels = self.decoder.convout.in_channels
        self.encoder.convin = nn.Sequential(nn.Conv2d(1, convin_out_channels, kernel_size=3, padding='same'), nn.ELU(inplace=True))
        self.decoder.convout = nn.Conv2d(convout_in_channels, 1, kernel_size=3, padding='same')

    def _features(self, audio):
        """The encoder input without its channel dim: magnitudes (B,F,T)."""
        return self.sliCQ.magnitude(audio)

    def encode(self, audio):
        """audio (B,1,N) -> (latents (B,D,T), embeddings, {}) from the (B,1,F,T) magnitude features."""
        return self.encoder(self._features(audio).unsqueeze(-3))

    def to_activations(self, coefficients):
        """logits (B,1,F,T) -> activations (B,F,T): tanh (reference modules.py:980-997)."""
        return ops.Activations1Fn.apply(coefficients.squeeze(-3))

    def sonify(self, coefficients, audio_init=None, n_iter=32, momentum=0.99):
        """magnitudes (B,1,F,T) as the model returns them -> audio (B,1,N) by phase retrieval (CQT.griffin_lim), inf-normalised as
        ``decode`` normalises.  ``audio_init``: the start of the iteration; the input mixture is the usual "mixture phase" choice."""
        return self.sliCQ.griffin_lim(coefficients, n_iter=n_iter, momentum=momentum, audio_init=audio_init)


class TimbreTrapMagDB(TimbreTrapMag):
    """
    Magnitude-CQT (decibels) variant (reference modules.py:1000-1075): the encoder takes CQT.to_decibels of the magnitudes (per clip,
    80 dB range, rescaled to [0, 1]: tt_decibels), the decoder's output goes through a sigmoid (fused like TimbreTrapMag's relu), and the
    activations are the squeezed logits themselves.
    """

    OUT_ACT = ACT_SIGMOID

    def _features(self, audio):
        return self.sliCQ.to_decibels(self.sliCQ.magnitude(audio))

    def to_activations(self, coefficients):
        """logits (B,1,F,T) -> activations (B,F,T): a view (reference modules.py:1058-1075)."""
        return coefficients.squeeze(-3)

    def sonify(self, coefficients, audio_init=None, n_iter=32, momentum=0.99):
        """rescaled decibels (B,1,F,T) as the model returns them -> audio (B,1,N): CQT.from_decibels, then TimbreTrapMag.sonify."""
        return TimbreTrapMag.sonify(self, self.sliCQ.from_decibels(coefficients), audio_init, n_iter, momentum)


class FiLM(nn.Module):
    """
    FiLM conditioning layer (reference modules.py:847-889): y = x * gamma(condition) + beta(condition) per channel of x (..., D, T), with
    gamma and beta nn.Linear(n_conditions, D) -- kept as PARAMETER CONTAINERS (the reference's keys, default initialisation and RNG
    order); the map itself is csrc/film.hip.  Two conditions only: the kernels serve the model's reconstruction / transcription switch.
    """

    def __init__(self, embedding_size, n_conditions):
        if n_conditions != 2:
            raise NotImplementedError('FiLM with %r conditions: the MI355X path implements the two-condition switch of TimbreTrapFiLM'
                                      % (n_conditions,))
        nn.Module.__init__(self)
        self.gamma = nn.Linear(n_conditions, embedding_size)
        self.beta = nn.Linear(n_conditions, embedding_size)

    def forward(self, x, condition):
        """x (..., D, T); condition: two values, as a host sequence or a tensor.  The kernel takes the condition BY VALUE: a host sequence
        or CPU tensor costs nothing, a device tensor is read back with one ``.tolist()`` -- a host synchronisation (TimbreTrapFiLM's own
        decode never passes one)."""
        if torch.is_tensor(condition):
            condition = condition.detach().reshape(-1).tolist()
        return ops.film_modulate(x, self.gamma.weight, self.gamma.bias, self.beta.weight, self.beta.bias, condition)
