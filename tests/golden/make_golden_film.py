"""
Generates tests/golden/film.npz from the REFERENCE's FiLM variant (modules.py:780-889), the way make_golden_variants.py records the
magnitude variants: the reference is imported with make_golden.install_stubs() (the stub CQT of tests/golden/stub_cqt.py, so no value
of the transform is pinned) and only its outputs are recorded.  Run once:

    python tests/golden/make_golden_film.py

Configurations: mc1 = model_complexity 1, latent 32; mc2skip = model_complexity 2, latent 128, skip connections.  latent_size is always
given: with latent_size=None the reference raises in its own constructor (modules.py:799).

Weights: the closed-form ones of every other fixture, with the FiLM parameters replaced and Decoder.convin's weight x 30
(tests/film_ref.py: fixture_overrides) -- under the plain closed-form weights the two conditions differ by 2e-5 of the output, so a
swapped or ignored condition would pass the 1e-4 comparison of the GPU test.  This script ASSERTS that reconstruction and transcription
are at least ten tolerances apart at both configurations.

Recorded:
  * initialisation under torch.manual_seed(0) at mc 1 and 2: keys, shapes and sums of every entry, decoder.convin.0.* and film_layer.*
    in full (at mc 2 every 4th input and output channel of the 1 MB decoder.convin.0.weight);
  * per configuration the five forward outputs (consistency on) and to_activations, the four losses and the total of the train.py step,
    the gradient of every parameter -- at mc1 the outputs in full (to_activations: every 2nd bin), at mc2skip (the size limit of a committed file) every 8th bin and 2nd
    frame plus sum and L2 norm; gradients as sum, L2 norm and first values, film_layer.* and decoder.convin.0.bias in full;
  * at mc1 chunked_inference for both switches and inference (every 12th bin), transcribe checked to be to_activations of the former;
  * the layer alone: film_layer(latents, condition) for both conditions and its input, in full -- the bit-exact pin.
"""

import io
import os
import sys
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import film_ref  # noqa: E402
import make_golden as mg  # noqa: E402
import stub_cqt  # noqa: E402

CONFIGS = (('mc1', dict(model_complexity=1, latent_size=32)),
           ('mc2skip', dict(model_complexity=2, latent_size=128, skip_connections=True)))
OUTPUTS = ('reconstruction', 'latents', 'transcription', 'transcription_rec', 'transcription_scr')
FULL_GRADS = ('film_layer.', 'decoder.convin.0.bias')


def stats(t):
    t = t.detach().double().flatten()
    return np.array([float(t.sum()), float(t.norm())], dtype=np.float64)


def sample(t):
    """What is kept of a (B, 2, F, T) output at mc2skip."""
    return mg.npy(t[:, :, ::8, ::2]) if t.dim() == 4 else mg.npy(t)


def save_npz(path, arrays):
    """np.savez_compressed with a fixed time stamp on every member: the same arrays give the same bytes on every run."""
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED) as z:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(name + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())


def main():
    mg.install_stubs()
    sys.path.insert(0, '/root/reference')
    import timbre_trap.framework as ref
    from timbre_trap.framework import objectives as robj
    torch.set_grad_enabled(True)
    npy = mg.npy
    out = {}
    secs = (mg.STUB_BLOCK + 0.5) / 22050

    # ---- initialisation: keys, shapes, default weights under a seed
    for mc, latent in ((1, 32), (2, 128)):
        torch.manual_seed(0)
        model = ref.TimbreTrapFiLM(22050, 9, 60, 3, latent_size=latent, model_complexity=mc)
        sd = model.state_dict()
        keys = [k for k in sd if not k.startswith('sliCQ.')]
        out['mc%d_keys' % mc] = np.array(keys)
        out['mc%d_shapes' % mc] = np.array([str(tuple(sd[k].shape)) for k in keys])
        out['mc%d_init_sums' % mc] = np.array([float(sd[k].double().sum()) for k in keys], dtype=np.float64)
        for k in keys:
            if k.startswith(('decoder.convin.0.', 'film_layer.')):
                # (mc 2: Decoder.convin's weight alone is 1 MB of noise -- every 4th input and output channel; its sum is above)
                out['mc%d_init.%s' % (mc, k)] = npy(sd[k][::4, ::4]) if (mc == 2 and k.endswith('convin.0.weight')) else npy(sd[k])

    # ---- behaviour on closed-form weights with distinct FiLM parameters, stub transform
    for tag, kw in CONFIGS:
        model = ref.TimbreTrapFiLM(22050, 9, 60, secs, **kw)
        assert model.sliCQ.block_length == mg.STUB_BLOCK
        sd = mg.load_closed_form(model)
        model.load_state_dict(film_ref.fixture_overrides(sd, kw['latent_size']))
        audio = stub_cqt.closed_form_audio(2, mg.STUB_BLOCK)
        res = model(audio, consistency=True)
        sep = film_ref.separation(res[0].detach(), res[2].detach())
        print('%s: reconstruction and transcription %.1f tolerances apart (%.2e of max |rec|)'
              % (tag, sep, float((res[0] - res[2]).detach().abs().max() / res[0].detach().abs().max())))
        assert sep >= 10, (tag, sep)
        out[f'{tag}_separation'] = np.float64(sep)
        for name, t in zip(OUTPUTS, res[:5]):
            out[f'{tag}_fwd_{name}'] = npy(t) if tag == 'mc1' else sample(t)
            out[f'{tag}_fwdstat_{name}'] = stats(t)
        act = model.to_activations(res[2])
        out[f'{tag}_act'] = npy(act[:, ::2]) if tag == 'mc1' else npy(act[:, ::8, ::2])
        out[f'{tag}_actstat'] = stats(act)

        # the layer alone, on the model's own latents
        latents = res[1].detach()
        out[f'{tag}_film_in'] = npy(latents)
        with torch.no_grad():
            for transcribe in (False, True):
                cond = torch.tensor([transcribe, not transcribe], dtype=latents.dtype)
                out[f'{tag}_film_out_t{int(transcribe)}'] = npy(model.film_layer(latents, cond))

        if tag == 'mc1':
            long_audio = stub_cqt.closed_form_audio(1, int(2.5 * mg.STUB_BLOCK))
            model.eval()
            with torch.no_grad():
                trn, rec = model.chunked_inference(long_audio, True), model.chunked_inference(long_audio, False)
                assert film_ref.separation(rec, trn) >= 10
                out[f'{tag}_chunked_trn'] = npy(trn[:, :, ::12])
                out[f'{tag}_chunked_rec'] = npy(rec[:, :, ::12])
                out[f'{tag}_inference'] = npy(model.inference(long_audio, False)[:, :, ::12])
                assert torch.equal(model.transcribe(long_audio), model.to_activations(trn))
            model.train()

        # the train.py step (:404-496)
        coeffs = model.sliCQ(audio)
        gt = stub_cqt.closed_form_targets(2, 540, mg.STUB_M)
        rec, lat, trn, trn_rec, trn_scr, _ = model(audio, True)
        l_rec = robj.compute_reconstruction_loss(rec, coeffs)
        l_trn = robj.compute_transcription_loss(model.to_activations(trn), gt, True)
        l_sp, l_sc = robj.compute_consistency_loss(trn_rec, trn_scr, trn)
        total = l_rec + l_trn + (l_sp + l_sc)
        model.zero_grad()
        total.backward()
        out[f'{tag}_losses'] = np.array([float(v.detach()) for v in (l_rec, l_trn, l_sp, l_sc, total)], dtype=np.float64)
        for k, p in model.named_parameters():
            g = p.grad.double().flatten()
            if k.startswith(FULL_GRADS):
                out[f'{tag}_grad.{k}'] = npy(p.grad)
            else:
                out[f'{tag}_gradstat.{k}'] = npy(torch.cat([g.sum().view(1), g.norm().view(1), g[:6]]))
    path = os.path.join(HERE, 'film.npz')
    save_npz(path, out)
    print('wrote %s: %d bytes' % (path, os.path.getsize(path)))


if __name__ == '__main__':
    main()
