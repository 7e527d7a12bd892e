"""Frames/s of the two fp32-storage modes, f32 (f32-input MFMA) and f32s (exact split products on the 16-bit MFMA), at the headline's conditions in ONE
session: conv5, batch 256, 256 x 256 uint8 frames resident in HBM, two lanes (the loop of scripts/variant_rates.py); then the per-launch times of the f32s
plan (pvr_encoder_profile, median of 5) with the fp32-equivalent TFLOP/s of every convolution, and both modes' parity against each other on one batch.
python scripts/precision_mode_rates.py [output file]        (profiles/f32s_rates.txt is a recording of this)
python scripts/precision_mode_rates.py vit [output file]    the ViT encoders' f16 and f32 plans instead (clip_b32, clip_b16, mae_b16: batch 64, uint8 frames of
                                                            the size the transform crops from resident in HBM, two lanes), and both plans' distance on one batch
                                                            (profiles/vit_f32_rates.txt holds a recording of this)"""
import ctypes as C
import os, sys, time
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pvr_habitat_amd import synth, _lib
from pvr_habitat_amd.embeddings import HipResNet50, lane_streams

lines = []
def say(s):
    print(s, flush=True)
    lines.append(s)

def vit_modes():
    n = 64
    streams = lane_streams()
    for variant, mk_sd, side in (('clip_b32', lambda: synth.clip_vit_state_dict(1, patch=32), 224), ('clip_b16', lambda: synth.clip_vit_state_dict(1, patch=16), 224),
                                 ('mae_b16', lambda: synth.mae_vit_state_dict(1), 256)):
        sd = mk_sd()
        pool = [torch.from_numpy(synth.smooth_frames(3 + i, n, side, side)).cuda() for i in range(2)]
        rate, first = {}, {}
        for dt in ('f16', 'f32'):
            m = HipResNet50(sd, variant, compute_dtype=dt, max_batch=n)
            outs = [torch.empty((n, m.out_size), device='cuda') for _ in range(2)]
            def run(steps):
                for s_ in streams: s_.wait_stream(torch.cuda.current_stream())
                for i in range(steps):
                    with torch.cuda.stream(streams[i & 1]):
                        m.forward_into(pool[i & 1], outs[i & 1], lane=i & 1)
                torch.cuda.synchronize()
            steps = 6 if dt == 'f32' else 30
            run(2)
            t0 = time.perf_counter(); run(steps); el = time.perf_counter() - t0
            rate[dt] = steps * n / el
            first[dt] = m(pool[0]).cpu().numpy().astype(np.float64)
            say('%-8s %-3s batch %d, %dx%d uint8 frames in HBM, two lanes: %8.0f frames/s (%.2f ms per batch)' % (variant, dt, n, side, side, rate[dt], el / steps * 1e3))
            m.close(); del m
        a, b = first['f16'], first['f32']
        say('%-8s f16 / f32 rate: %.1fx;  f16 against f32 on one batch of %d: rel-L2 %.2e max-norm %.2e'
            % (variant, rate['f16'] / rate['f32'], n, np.linalg.norm(a - b) / np.linalg.norm(b), np.abs(a - b).max() / np.abs(b).max()))

if sys.argv[1:2] == ['vit']:
    vit_modes()
    if len(sys.argv) > 2:
        with open(sys.argv[2], 'w') as f:
            f.write('\n'.join(lines) + '\n')
    sys.exit(0)

N = 256
sd = synth.resnet50_state_dict(2, 'conv5')
pool = [torch.from_numpy(synth.frames(3 + i, N, 256, 256)).cuda() for i in range(4)]
streams = lane_streams()
rate, first = {}, {}
for dt in ('f32', 'f32s', 'f16'):
    m = HipResNet50(sd, 'conv5', compute_dtype=dt, max_batch=N)
    outs = [torch.empty((N, m.out_size), device='cuda') for _ in range(2)]
    def run(steps):
        for s_ in streams: s_.wait_stream(torch.cuda.current_stream())
        for i in range(steps):
            with torch.cuda.stream(streams[i & 1]):
                m.forward_into(pool[i % 4], outs[i & 1], lane=i & 1)
        torch.cuda.synchronize()
    steps = 12 if dt == 'f32' else 40
    run(4)
    t0 = time.perf_counter(); run(steps); el = time.perf_counter() - t0
    rate[dt] = steps * N / el
    first[dt] = m(pool[0]).cpu().numpy().astype(np.float64)
    say('conv5 %-4s batch %d, 256x256 uint8 frames in HBM, two lanes: %8.0f frames/s (%.2f ms per batch)' % (dt, N, rate[dt], el / steps * 1e3))
    if dt == 'f32s':
        cap = 128
        op_ms = (C.c_float * cap)(); op_fl = (C.c_double * cap)(); n_ops = C.c_int32()
        acc = []
        for r in range(5):
            _lib.check(_lib.lib().pvr_encoder_profile(m._handle, C.c_void_p(pool[r % 4].data_ptr()), N, 256, 256, C.c_void_p(outs[0].data_ptr()), outs[0].stride(0),
                                                      _lib.stream_ptr(), op_ms, op_fl, cap, C.byref(n_ops)))
            acc.append(np.array(op_ms[:n_ops.value]))
        med = np.median(np.stack(acc), axis=0)
        names = ['preprocess+normalize', 'stem_split16', 'maxpool'] + m.op_names() + ['pool/flatten']
        say('f32s plan, per launch (pvr_encoder_profile, one lane, median of 5; TFLOP/s = fp32-equivalent, 2 M K Cout / time):')
        for i in range(n_ops.value):
            say('  %-28s %8.4f ms %s' % (names[i], med[i], ('%7.1f TFLOP/s' % (op_fl[i] / med[i] / 1e9)) if op_fl[i] > 0 else ''))
        say('  %-28s %8.4f ms (%.0f frames/s on one lane with the events in)' % ('total', med.sum(), N / med.sum() * 1e3))
    m.close(); del m
say('f32s / f32 rate: %.2fx   (f16 default plan / f32s: %.2fx)' % (rate['f32s'] / rate['f32'], rate['f16'] / rate['f32s']))
a, b = first['f32s'], first['f32']
say('f32s vs f32 on one batch of %d: rel-L2 %.2e max-norm %.2e' % (N, np.linalg.norm(a - b) / np.linalg.norm(b), np.abs(a - b).max() / np.abs(b).max()))
if len(sys.argv) > 1:
    with open(sys.argv[1], 'w') as f:
        f.write('\n'.join(lines) + '\n')
