"""dx of the block-backward kernels at the bench's launch shapes, as SHA-256 per case, for a bit-for-bit comparison of two builds.

    TTRAP_LIB=libttrap_<a>.so python tools/bwd_loops_same.py dump a.json      # one process per library (tools/build_variant.sh)
    TTRAP_LIB=libttrap_<b>.so python tools/bwd_loops_same.py dump b.json
    python tools/bwd_loops_same.py compare a.json b.json                      # exit status 1 if any case differs
    python tools/bwd_loops_same.py compare-steps DIR_A DIR_B                  # two `bench.py --dump-outputs` directories

Cases: C = 16 (strips), 32 (k_wrb_bwd_a + k_wrb_dxw), 8 and 4 (k_nrb_bwd_fused) x dilation 1, 2, 3 plain (tt_wide_rb_bwd), dilation 1 gated
(tt_wide_level_bwd_gated) and riding (tt_wide_level_bwd_gated_join, two batches), bf16 and fp16.  Inputs are seeded; h1 comes from the
library's own forward."""
import ctypes
import hashlib
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'timbre-trap_amd'))

SHAPES = {16: (3, 133, 1024), 32: (4, 65, 1024), 8: (2, 269, 1024), 4: (2, 540, 1024)}


def dump(path):
    import torch
    from timbre_trap._hip import check, ptr, stream_ptr
    from timbre_trap.framework import ops

    def rand(*shape, seed, scale=1.0):
        g = torch.Generator().manual_seed(seed)
        return ((torch.rand(*shape, generator=g) * 2 - 1) * scale).cuda().contiguous()

    out = {}
    for elt, ELT in (('bf16', torch.bfloat16), ('fp16', torch.float16)):
        lib, st = ops.lib16(ELT), stream_ptr()
        for C, (B, H, T) in SHAPES.items():
            nhwc = lambda b=B: torch.empty((b, H, T, C), dtype=ELT, device='cuda')
            xb, gb, sgb = nhwc(), nhwc(), nhwc(2 * B)
            check(lib.tt_wide_pack(ptr(rand(B, C, H, T, seed=1)), ptr(xb), B, C, H, T, st), 'pack')
            check(lib.tt_wide_pack(ptr(rand(B, C, H, T, seed=6)), ptr(gb), B, C, H, T, st), 'pack')
            check(lib.tt_wide_pack(ptr(rand(2 * B, C, H, T, seed=7, scale=0.7)), ptr(sgb), 2 * B, C, H, T, st), 'pack')
            w1, b1 = rand(C, C, 3, 3, seed=2, scale=1.0 / (3 * C ** 0.5)), rand(C, seed=3, scale=0.3)
            w2, b2 = rand(C, C, 1, 1, seed=4, scale=1.0 / C ** 0.5), rand(C, seed=5, scale=0.3)
            sw = torch.tensor([0.5, -1.25, 2.0, 0.75, 1.5]).cuda()
            ws = torch.zeros(max(lib.tt_wide_scratch_bytes(B, C, H, T), lib.tt_wide_level_scratch_bytes(1, B, C, H, T)), dtype=torch.uint8, device='cuda')
            one = lambda t: (ctypes.c_void_p * 1)(t.data_ptr())
            for d in (1, 2, 3):
                yb, hb = nhwc(), nhwc()
                check(lib.tt_wide_rb_fwd(ptr(xb), ptr(w1), ptr(b1), ptr(w2), ptr(b2), ptr(yb), ptr(hb), B, C, H, T, d, st), 'fwd')
                for form in (('plain', 'gated', 'riding') if d == 1 else ('plain',)):
                    dx = nhwc()
                    g = [torch.zeros(s, device='cuda') for s in ((C, C, 3, 3), (C,), (C, C, 1, 1), (C,))]
                    if form == 'plain':
                        check(lib.tt_wide_rb_bwd(ptr(xb), ptr(hb), ptr(gb), ptr(w1), ptr(w2), ptr(b2), ptr(dx), ptr(g[0]), ptr(g[1]), ptr(g[2]), ptr(g[3]),
                                                 ptr(ws), B, C, H, T, d, st), 'bwd')
                    else:
                        args = (1, one(xb), one(hb), ptr(gb), one(w1), one(w2), one(b2), ptr(dx), None, None, one(g[0]), one(g[1]), one(g[2]), one(g[3]),
                                ptr(ws), B, C, H, T, (ctypes.c_int * 1)(d))
                        if form == 'gated':
                            check(lib.tt_wide_level_bwd_gated(*args, st), 'gated')
                        else:
                            ds = torch.zeros(5, device='cuda')
                            rc = lib.tt_wide_level_bwd_gated_join(*args, ptr(sgb), 2, ptr(sw), 3, ptr(ds), st)
                            if rc != 0:                      # 1: no riding form on this dispatch (C = 32 strips) -- not a case
                                continue
                    torch.cuda.synchronize()
                    out['%s C=%d d=%d %s' % (elt, C, d, form)] = hashlib.sha256(dx.view(torch.int16).cpu().numpy().tobytes()).hexdigest()
    json.dump(out, open(path, 'w'), indent=1, sort_keys=True)
    print('%d cases -> %s (%s)' % (len(out), path, os.environ.get('TTRAP_LIB', 'default library')))


def compare(a, b):
    da, db = json.load(open(a)), json.load(open(b))
    diff = sorted(k for k in set(da) | set(db) if da.get(k) != db.get(k))
    print('%d cases, dx bit-identical in %d' % (len(set(da) | set(db)), len(set(da) | set(db)) - len(diff)))
    for k in diff:
        print('DIFFERS: %s' % k)
    return 1 if diff else 0


def compare_steps(a, b):
    """two `bench.py --dump-outputs` directories: loss terms bit for bit, flat_grad within the run-to-run bound of
    tests/test_gpu_model.py::test_run_to_run_reproducibility_bounds (2e-5 of the largest element)."""
    import numpy as np
    bad = 0
    for name in ('loss_total', 'loss_reconstruction', 'loss_transcription', 'loss_consistency_spectral', 'loss_consistency_score'):
        x, y = np.load(os.path.join(a, name + '.npy')), np.load(os.path.join(b, name + '.npy'))
        same = x.tobytes() == y.tobytes()
        bad += not same
        print('%-28s %s  %r %r' % (name, 'equal bit for bit' if same else 'DIFFERS', float(x[0]), float(y[0])))
    x, y = np.load(os.path.join(a, 'flat_grad.npy')).astype(np.float64), np.load(os.path.join(b, 'flat_grad.npy')).astype(np.float64)
    err, bound = float(np.abs(x - y).max()), 2e-5 * float(np.abs(y).max())
    bad += not err <= bound
    print('%-28s max |a - b| %.3e, bound %.3e (%d elements, %d equal bit for bit)' % ('flat_grad', err, bound, x.size, int((x == y).sum())))
    return 1 if bad else 0


if __name__ == '__main__':
    if sys.argv[1] == 'dump':
        sys.exit(dump(sys.argv[2]))
    sys.exit(compare(sys.argv[2], sys.argv[3]) if sys.argv[1] == 'compare' else compare_steps(sys.argv[2], sys.argv[3]))
