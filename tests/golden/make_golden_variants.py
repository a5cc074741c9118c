"""
Generates tests/golden/variants.npz from the REFERENCE's magnitude variants (modules.py:892-1075), the way make_golden.py records
TimbreTrap: the reference is imported with make_golden.install_stubs() (the stub CQT of tests/golden/stub_cqt.py, so no value of
the transform itself is pinned) and the outputs are recorded on closed-form weights and inputs.  Run once:

    python tests/golden/make_golden_variants.py

torchaudio is absent: ``AmplitudeToDB('amplitude', top_db=80)`` -- what the reference's CQT.to_decibels calls per clip
(cqtwrapper.py:143-182) -- is restated here from torchaudio's published definition:
    d = 20 log10(max(m, 1e-10));  d = max(d, max(d) - top_db)     (max over the whole tensor it is given: one clip)
Recorded per variant (Mag, MagDB) at model_complexity 1 and at 2 with latent 128 and skip connections:
  the five forward outputs (consistency on), to_activations, the four losses of the train.py step (the reconstruction target built as
  train.py:406-413 does), gradients (the edge layers' in full at mc 1; sum, L2 norm and first
  values of every other one), inference and chunked_inference at mc 1 (channel 0 of its two equal channels; transcribe is
  checked to be to_activations of it); and for the initialisation: state_dict keys and shapes, and the default initial weights' statistics under a seed.
"""

import os
import sys

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402
import stub_cqt  # noqa: E402


class AmplitudeToDB(nn.Module):
    """torchaudio.transforms.AmplitudeToDB restated for stype='amplitude' (multiplier 20, amin 1e-10, ref 1, db_multiplier 0)."""

    def __init__(self, stype='power', top_db=None):
        super().__init__()
        self.multiplier = 10.0 if stype == 'power' else 20.0
        self.top_db = top_db

    def forward(self, x):
        d = self.multiplier * torch.log10(torch.clamp(x, min=1e-10))
        if self.top_db is not None:
            d = torch.max(d, d.max() - self.top_db)
        return d


def main():
    mg.install_stubs()
    sys.modules['torchaudio.transforms'].AmplitudeToDB = AmplitudeToDB
    sys.path.insert(0, '/root/reference')
    import timbre_trap.framework as ref
    from timbre_trap.framework import objectives as robj
    torch.set_grad_enabled(True)
    npy = mg.npy
    out = {}
    secs = (mg.STUB_BLOCK + 0.5) / 22050
    for cls_name in ('TimbreTrapMag', 'TimbreTrapMagDB'):
        cls = getattr(ref, cls_name)
        # ---- initialisation: keys, shapes, default weights under a seed (no stub needed for the values: nn defaults)
        for mc in (1, 2):
            torch.manual_seed(0)
            model = cls(22050, 9, 60, 3, model_complexity=mc)
            sd = model.state_dict()
            keys = [k for k in sd if not k.startswith('sliCQ.')]
            out['%s_mc%d_keys' % (cls_name, mc)] = np.array(keys)
            out['%s_mc%d_shapes' % (cls_name, mc)] = np.array([str(tuple(sd[k].shape)) for k in keys])
            out['%s_mc%d_init_sums' % (cls_name, mc)] = np.array([float(sd[k].double().sum()) for k in keys], dtype=np.float64)
            for k in ('encoder.convin.0.weight', 'encoder.convin.0.bias', 'decoder.convout.weight', 'decoder.convout.bias'):
                out['%s_mc%d_init.%s' % (cls_name, mc, k)] = npy(sd[k])

        # ---- behaviour on closed-form weights, stub transform
        for tag, kw in (('mc1', dict(model_complexity=1)),
                        ('mc2skip', dict(model_complexity=2, latent_size=128, skip_connections=True))):
            model = cls(22050, 9, 60, secs, **kw)
            assert model.sliCQ.block_length == mg.STUB_BLOCK
            mg.load_closed_form(model)
            pre = '%s_%s' % (cls_name, tag)
            audio = stub_cqt.closed_form_audio(2, mg.STUB_BLOCK)
            res = model(audio, consistency=True)
            for name, t in zip(('reconstruction', 'latents', 'transcription', 'transcription_rec', 'transcription_scr'), res[:5]):
                out[f'{pre}_fwd_{name}'] = npy(t)
            out[f'{pre}_act'] = npy(model.to_activations(res[2]))
            if tag == 'mc1':                             # (the size limit of a committed file: inference at mc 1 only)
                long_audio = stub_cqt.closed_form_audio(1, int(2.5 * mg.STUB_BLOCK))
                model.eval()
                with torch.no_grad():
                    # chunked_inference returns two equal channels (1-channel chunks broadcast into a 2-channel buffer): one is kept
                    trn, rec = model.chunked_inference(long_audio, True), model.chunked_inference(long_audio, False)
                    assert trn.size(1) == 2 and torch.equal(trn[:, 0], trn[:, 1]) and torch.equal(rec[:, 0], rec[:, 1])
                    out[f'{pre}_chunked_trn'] = npy(trn[:, :1])
                    out[f'{pre}_chunked_rec'] = npy(rec[:, :1])
                    out[f'{pre}_inference'] = npy(model.inference(long_audio, False))
                    # transcribe = to_activations(chunked_inference(audio, True)): tanh of both channels (Mag), the buffer (MagDB)
                    tr = model.transcribe(long_audio)
                    assert tr.shape == trn.shape and torch.equal(tr, model.to_activations(trn))
            model.train()

            # the train.py step (:404-496) with the reconstruction target of :406-413
            coeffs = model.sliCQ(audio)
            coeffs = model.sliCQ.to_magnitude(coeffs).unsqueeze(-3)
            if cls_name == 'TimbreTrapMagDB':
                coeffs = model.sliCQ.to_decibels(coeffs)
            gt = stub_cqt.closed_form_targets(2, 540, mg.STUB_M)
            rec, lat, trn, trn_rec, trn_scr, _ = model(audio, True)
            act = model.to_activations(trn)
            l_rec = robj.compute_reconstruction_loss(rec, coeffs)
            l_trn = robj.compute_transcription_loss(act, gt, True)
            l_sp, l_sc = robj.compute_consistency_loss(trn_rec, trn_scr, trn)
            total = l_rec + l_trn + (l_sp + l_sc)
            model.zero_grad()
            total.backward()
            out[f'{pre}_losses'] = np.array([float(l_rec), float(l_trn), float(l_sp), float(l_sc), float(total)], dtype=np.float64)
            for k, p in model.named_parameters():
                g = p.grad.double().flatten()
                if tag == 'mc1' and k.startswith(('encoder.convin', 'decoder.convout')):
                    out[f'{pre}_grad.{k}'] = npy(p.grad)
                else:
                    out[f'{pre}_gradstat.{k}'] = npy(torch.cat([g.sum().view(1), g.norm().view(1), g[:6]]))
    np.savez_compressed(os.path.join(HERE, 'variants.npz'), **out)


if __name__ == '__main__':
    main()
