"""EmbeddingNet / UberModel / EmbeddingWrapper with the reference call surface, HIP inside.

Mirrors reference src/embeddings.py:
  * `_get_embedding(name, in_channels, pretrained, train)`  (:60-332)  name registry + transforms
  * `UberModel`                                              (:44-57)   concat of separate models
  * `EmbeddingNet(embedding_name, in_channels=3, pretrained=True, train=False, disable_cuda=False)`
    `.forward(uint8 (N,H,W,3)) -> np.float32 (N,O).squeeze()`  (:339-402)
  * `EmbeddingWrapper.observation`                           (:441-444)
and the checkpoint loaders of src/vision_models/moco.py:6-113 / resnet.py:6-104 (key remapping and
their asserts).  All arithmetic (transforms + network) runs in libpvr_hip.so on the MI355X; this
module only owns names, state_dicts and tensors.  `disable_cuda=True` selects the library's host backend (ResNet family, fp32 C++ loops);
without that flag there is no CPU path: a
box without a GPU raises instead of silently computing something else.
"""
import ctypes as C
import os
import time
import weakref
import zlib

import numpy as np
import torch
import torch.nn as nn

from . import _lib, synth

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)
CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)
OUT_SIZE = {'r18': 512, 'r34': 512, 'conv5': 2048, 'conv4': 2058, 'conv3': 2156, 'clip_b32': 512, 'clip_b16': 512, 'mae_b16': 768, 'mae_l16': 1024, 'mae_h14': 1280, 'clip_rn50': 1024, 'random5': 1568}
_ARCH = {'conv5': _lib.ARCH_RESNET50, 'conv4': _lib.ARCH_RESNET50_L4, 'conv3': _lib.ARCH_RESNET50_L3,
         'clip_b32': 3, 'clip_b16': 4, 'mae_b16': 5, 'random5': 6, 'mae_l16': 7, 'mae_h14': 8, 'clip_rn50': 9, 'r18': 10, 'r34': 11}

# ---------------------------------------------------------------------------------------------
# name registry (reference src/embeddings.py:113-280): name -> (loader family, variant, checkpoint)
# ---------------------------------------------------------------------------------------------
_SINGLE = {
    'resnet18': ('torchvision', 'r18', None),        # embeddings.py:112-117
    'resnet34': ('torchvision', 'r34', None),
    'resnet50': ('torchvision', 'conv5', None),
    'resnet50_places': ('resnet', 'conv5', 'resnet50_places.pth.tar'),
    'resnet50_l4': ('resnet', 'conv4', 'resnet50_l4.pth.tar'),
    'resnet50_l3': ('resnet', 'conv3', 'resnet50_l3.tar'),
    'resnet50_places_l4': ('resnet', 'conv4', 'resnet50_places_l4.tar'),
    'resnet50_places_l3': ('resnet', 'conv3', 'resnet50_places_l3.tar'),
    'demy': ('moco', 'conv5', 'demy.pth'),
    'moco_aug': ('moco', 'conv5', 'moco_aug.pth.tar'),
    'moco_aug_habitat': ('moco', 'conv5', 'moco_aug_habitat_64.pth'),
    'moco_aug_mujoco': ('moco', 'conv5', 'moco_aug_mujoco.pth'),
    'moco_aug_uber': ('moco', 'conv5', 'moco_aug_uber.pth'),
    'moco_aug_places': ('moco', 'conv5', 'moco_aug_places.pth.tar'),
    'moco_aug_l4': ('moco', 'conv4', 'moco_aug_l4.pth'),
    'moco_aug_places_l4': ('moco', 'conv4', 'moco_aug_places_l4.pth'),
    'moco_aug_l3': ('moco', 'conv3', 'moco_aug_l3.pth'),
    'moco_aug_places_l3': ('moco', 'conv3', 'moco_aug_places_l3.pth'),
    'moco_croponly': ('moco', 'conv5', 'moco_croponly.pth'),
    'moco_croponly_places': ('moco', 'conv5', 'moco_croponly_places.pth'),
    'moco_croponly_habitat': ('moco', 'conv5', 'moco_croponly_habitat_64.pth'),
    'moco_croponly_mujoco': ('moco', 'conv5', 'moco_croponly_mujoco.pth'),
    'moco_croponly_uber': ('moco', 'conv5', 'moco_croponly_uber.pth'),
    'moco_croponly_l4': ('moco', 'conv4', 'moco_croponly_l4.pth'),
    'moco_croponly_l3': ('moco', 'conv3', 'moco_croponly_l3.pth'),
    'moco_croponly_places_l4': ('moco', 'conv4', 'moco_croponly_places_l4.pth'),
    'moco_croponly_places_l3': ('moco', 'conv3', 'moco_croponly_places_l3.pth'),
    'moco_coloronly': ('moco', 'conv5', 'moco_coloronly.pth'),
}
_UBER = {}
for _base in ('moco_aug_places', 'moco_aug', 'moco_croponly_places', 'moco_croponly'):
    _m = {'3': _base + '_l3', '4': _base + '_l4', '5': _base}
    for _combo in ('345', '35', '34', '45'):
        _UBER['%s_uber_%s' % (_base, _combo)] = [_m[c] for c in _combo]      # embeddings.py:195-280
# names the reference registers but whose model families are not built yet
_NOT_BUILT = ('maskrcnn_l3',)
# CLIP visual towers: 'clip_vit' is the reference's name (ViT-B/32, embeddings.py:303-304); 'clip_vit_b16' is the
# same block layout at patch 16 (BASELINE config 3), not a reference registry name
_CLIP = {'clip_vit': ('clip_b32', 'ViT-B-32.pt', 32), 'clip_vit_b16': ('clip_b16', 'ViT-B-16.pt', 16),
         'clip_rn50': ('clip_rn50', 'RN50.pt', 0)}            # embeddings.py:305-306 (ModifiedResNet-50 + attention pool)


def _dtype_from_env(compute_dtype=None):
    # Default f16 (round 5): the reference is fp32 and the north star asks for embeddings within 1e-3 of it; f16 storage (11-bit significand)
    # measures 4e-4 at the same rate as bf16 (8-bit significand, 3e-3).  A checkpoint whose activations leave f16's range raises
    # FloatingPointError naming compute_dtype='bf16' as the way out: every output batch is checked for non-finite values (_checked / the device flag of
    # stream_embed), and - because an overflow INSIDE the network can be turned into a finite value by the next ReLU - the first frames a net embeds run
    # once through pvr_encoder_check_range, which checks every convolution's output (EmbeddingNet.validate_range).  Later batches rely on the output check.
    d = (compute_dtype or os.environ.get('PVR_DTYPE', 'f16')).lower()
    if d in ('bf16', 'bfloat16'):
        return _lib.PVR_BF16
    if d in ('f16', 'fp16', 'float16', 'half'):
        return _lib.PVR_F16
    if d in ('f32', 'fp32', 'float32'):
        return _lib.PVR_F32                     # reference-precision mode (ResNet family, CLIP / MAE ViT): fp32 storage, f32-input MFMA, a fraction of the 16-bit rate
    if d in ('f32s', 'f32_split'):
        # fp32 storage as 'f32', every product on the 16-bit MFMA as an exact (hi, lo) f16 split product: ~1e-6 from 'f32' at several times its rate.  The
        # high part is an f16, so activations must stay below 65504 (validate_range checks the first frames; 'f32' has the full range)
        return _lib.PVR_F32S
    raise ValueError('compute dtype must be bf16, f16, f32 or f32s, got %r' % d)


# ---------------------------------------------------------------------------------------------
# checkpoint -> torchvision-named state_dict (reference moco.py / resnet.py key handling)
# ---------------------------------------------------------------------------------------------
def _expected_keys(variant):
    return [k for k in synth.resnet50_state_dict(0, variant, keys_only=True)]


def remap_checkpoint(state_dict, family, variant):
    """Apply the reference loaders' key remapping and asserts; returns {torchvision key: tensor}.

    moco:   keep 'module.encoder_q.*' except 'module.encoder_q.fc*', strip the prefix (moco.py:14-21)
    resnet: strip 'module.' (resnet.py:33-38, 95-99)
    For the compressed variants the checkpoint stores the nn.Sequential nesting
    ('layer4.0.<i>...', 'layer4.1....') because it was saved from the edited model."""
    out = {}
    for k, v in state_dict.items():
        if family == 'moco':
            if k.startswith('module.encoder_q') and not k.startswith('module.encoder_q.fc'):
                out[k[len('module.encoder_q.'):]] = v
        else:
            if k.startswith('module.'):
                out[k[len('module.'):]] = v
    want = _expected_keys(variant)
    missing = [k for k in want if k not in out]
    unexpected = [k for k in out if k not in set(want)]
    if family == 'moco' or variant == 'conv5':
        assert len(missing) == 0, 'missing keys: %s' % missing[:5]                 # moco.py:24, resnet.py:102
    if variant == 'conv3':
        assert all(('fc.' in n or 'layer4.' in n or 'layer3.2' in n) for n in unexpected)   # moco.py:67
    if variant == 'conv4':
        assert all(('fc.' in n or 'layer4.2' in n) for n in unexpected)           # moco.py:110
    return {k: out[k] for k in want if k in out}


def _find_checkpoint(path):
    for d in ('.', os.environ.get('PVR_CHECKPOINT_DIR', '')):
        if d and os.path.isfile(os.path.join(d, path)):
            return os.path.join(d, path)
    return None


def _load_named_state_dict(name, pretrained):
    family, variant, ckpt = _SINGLE[name]
    synthetic_ok = os.environ.get('PVR_SYNTHETIC_WEIGHTS', '0') == '1'
    seed = zlib.crc32(name.encode()) & 0x7fffffff
    if family == 'torchvision':
        # torchvision hub weights cannot be downloaded here; a local torchvision-format file is used if present
        f = _find_checkpoint(name + '.pth') if pretrained else None
        if f is not None:
            sd = torch.load(f, map_location='cpu')
            return {k: v for k, v in sd.items() if not k.startswith('fc.')}, variant
        if pretrained and not synthetic_ok:
            raise FileNotFoundError("pretrained torchvision weights: put '" + name + ".pth' in . or "
                                    "$PVR_CHECKPOINT_DIR (no network), or set PVR_SYNTHETIC_WEIGHTS=1")
        return synth.resnet50_state_dict(seed, variant), variant
    f = _find_checkpoint(ckpt)
    if f is None:
        if synthetic_ok:
            return synth.resnet50_state_dict(seed, variant), variant
        raise FileNotFoundError(ckpt)          # what torch.load(checkpoint_path) raises in the reference
    checkpoint = torch.load(f, map_location=torch.device('cpu'))
    return remap_checkpoint(checkpoint['state_dict'], family, variant), variant


# ---------------------------------------------------------------------------------------------
# module tree holding torchvision-named tensors, so state_dict() keys equal the reference's
# ---------------------------------------------------------------------------------------------
class _Node(nn.Module):
    pass


def _install(root, key, tensor):
    parts = key.split('.')
    node = root
    for p in parts[:-1]:
        if p not in node._modules:
            node.add_module(p, _Node())
        node = node._modules[p]
    leaf = parts[-1]
    if leaf in ('running_mean', 'running_var', 'num_batches_tracked'):
        node.register_buffer(leaf, tensor)
    elif leaf in node._modules:                      # e.g. 'visual.proj' next to nothing else: keep as parameter
        raise KeyError(key)
    else:
        node.register_parameter(leaf, nn.Parameter(tensor, requires_grad=False))


class HipResNet50(_Node):
    """One frozen encoder: fp32 host tensors under the reference's state_dict names + a libpvr_hip encoder handle.
    variant: 'conv5' | 'conv4' | 'conv3' (ResNet50 family, torchvision names) or 'clip_b32' | 'clip_b16'
    (openai/CLIP visual tower, `visual.*` names)."""

    def __init__(self, state_dict, variant='conv5', compute_dtype=None, max_batch=None, chunk=None, host=False):
        super().__init__()
        self.variant = variant
        self._host = bool(host)                   # CPU plan of the library (pvr_encoder_set_host_backend): host tensors in and out, fp32
        self.out_size = OUT_SIZE[variant]
        self._clip = variant.startswith('clip')
        self._mae = variant.startswith('mae')
        self._dtype = _dtype_from_env(compute_dtype)
        self._max_batch = int(max_batch or os.environ.get('PVR_MAX_BATCH', 256))
        self._chunk = int(chunk or os.environ.get('PVR_CHUNK', 0))
        self._handle = None
        for k, v in state_dict.items():
            t = v if isinstance(v, torch.Tensor) else torch.from_numpy(np.asarray(v))
            _install(self, k, t.detach().clone().cpu())
        self.train(False)

    # -- encoder lifetime ----------------------------------------------------------------------
    def _release(self):
        if self._handle is not None:
            _lib.lib().pvr_encoder_destroy(self._handle)
            self._handle = None

    def close(self):
        """Free the library handle (folded weights, workspaces) NOW, at a point the caller chooses, instead of whenever the garbage
        collector finds the object.  The module stays usable: the next call re-folds and re-uploads from the host tensors."""
        self._release()

    def __del__(self):
        try:
            self._release()
        except Exception:
            pass

    def load_state_dict(self, *a, **k):
        r = super().load_state_dict(*a, **k)
        self._release()                       # re-fold / re-upload on next use
        return r

    def _build(self):
        L = _lib.lib()
        if self._host and (self._clip or self._mae or self.variant == 'random5'):
            raise NotImplementedError("host backend (disable_cuda / no GPU): only the torchvision ResNet family has a CPU plan, not '%s'" % self.variant)
        tr = transforms_for('clip' if self._clip else 'mae' if self._mae else '')     # (the interpolation mode follows from the arch)
        desc = _lib.EncoderDesc(arch=_ARCH[self.variant], dtype=_lib.PVR_F32 if self._host else self._dtype, max_batch=self._max_batch,
                                chunk=self._chunk, resize=tr.resize, crop=tr.crop)
        desc.mean[:] = tr.mean                                             # embeddings.py:313 / :84
        desc.std_[:] = tr.std
        h = C.c_void_p()
        _lib.check(L.pvr_encoder_create(C.byref(desc), C.byref(h)))
        try:
            if self._host:
                _lib.check(L.pvr_encoder_set_host_backend(h, 1))
            for k, v in self.state_dict().items():
                if k.endswith('num_batches_tracked'):
                    continue
                a = np.ascontiguousarray(v.detach().cpu().numpy(), dtype=np.float32)
                shp = (C.c_int64 * max(a.ndim, 1))(*(a.shape or (1,)))
                _lib.check(L.pvr_encoder_load_weights(h, k.encode(), a.ctypes.data_as(C.c_void_p), shp, a.ndim))
            _lib.check(L.pvr_encoder_finalize(h))
        except Exception:
            L.pvr_encoder_destroy(h)
            raise
        self._handle = h
        if self._host:
            return
        if getattr(self, '_low_latency', False):
            self.set_low_latency(True)

    @property
    def max_batch(self):
        return self._max_batch

    @property
    def lanes(self):
        """activation workspaces that can be in flight at once (the 'random' plan has a single workspace)"""
        return 1 if self.variant == 'random5' else 4

    def forward_into(self, frames_u8, out, lane=0):
        """frames_u8: cuda uint8 (N,H,W,3) contiguous; out: cuda fp32 2-D view with row stride out.stride(0).
        lane selects one of the activation workspaces: forwards on different lanes may be in flight at once on different
        streams (pvr_encoder_forward_lane); same-lane forwards issued on different streams are chained by the library
        (a per-lane event), so a workspace is never shared by two forwards in flight."""
        if not self._host:
            _lib.require_gpu()
        if self._handle is None:
            self._build()
        n, h, w, c = frames_u8.shape
        assert c == 3 and frames_u8.dtype == torch.uint8 and frames_u8.is_contiguous()
        assert out.dtype == torch.float32 and out.stride(1) == 1 and out.shape[1] == self.out_size
        if self._host:
            assert not frames_u8.is_cuda and not out.is_cuda, 'host-backend encoder: frames and output live in host memory'
        L = _lib.lib()
        for i in range(0, n, self._max_batch):
            m = min(self._max_batch, n - i)
            _lib.check(L.pvr_encoder_forward_lane(self._handle, lane, C.c_void_p(frames_u8[i:i + m].data_ptr()), m, h, w,
                                                  C.c_void_p(out[i:i + m].data_ptr()), out.stride(0), None if self._host else _lib.stream_ptr()))

    def op_names(self):
        """conv launches of the current HIP plan, in launch order (fused bottleneck tails read 'a.conv2+conv3+b.conv1')."""
        if self._handle is None:
            self._build()
        names, buf, i = [], C.create_string_buffer(256), 3
        while _lib.lib().pvr_encoder_launch_name(self._handle, i, buf, 256) > 0:
            names.append(buf.value.decode())
            i += 1
        return [n for n in names if n != 'pool/flatten']

    def kernel_names(self, n=None):
        """the kernel family each conv launch of the plan runs as in a forward of n frames (default: max_batch), in launch order:
        'bneck_frame(front1)', 'conv_wfrag(pool)', 'conv_pp256(dual)', 'chain', 'conv_split16', 'conv' ... (pvr_encoder_launch_kernel)"""
        if self._handle is None:
            self._build()
        names, buf, i = [], C.create_string_buffer(64), 3
        while _lib.lib().pvr_encoder_launch_kernel(self._handle, int(n or self._max_batch), i, buf, 64) > 0:
            names.append(buf.value.decode())
            i += 1
        return names

    def set_switch(self, name, value):
        """run-time A/B switches of the built plan: 'pool_fuse', 'stem_u8', 'frame_min_n', 'frame_run', 'frame_stagger', 'conv_algo',
        'stem_regpool' (pvr_encoder_debug_set_switch); every other PVR_* switch is read from the environment when the handle is created"""
        if self._handle is None:
            self._build()
        _lib.check(_lib.lib().pvr_encoder_debug_set_switch(self._handle, name.encode(), int(value)))

    def check_range(self, frames_u8):
        """Load-time validation of the 16-bit storage range on real frames (pvr_encoder_check_range): one forward of the UNFUSED plan with every launch's
        output checked for inf / NaN - an overflow inside the network can be turned into a finite, wrong embedding by the next ReLU, which the finite check of
        the output cannot see.  Returns the name of the first convolution whose output is non-finite, or None.  ResNet family, 16-bit plans - and 'f32s' plans,
        where an output above 65504 in magnitude counts as well: the next convolution rounds the high part of its operand to f16."""
        if self._handle is None:
            self._build()
        n = min(int(frames_u8.shape[0]), self._chunk or self._max_batch)
        fr = frames_u8[:n].contiguous()
        out = torch.empty((n, self.out_size), dtype=torch.float32, device=fr.device)
        bad = C.c_int32(-1)
        _lib.check(_lib.lib().pvr_encoder_check_range(self._handle, C.c_void_p(fr.data_ptr()), n, fr.shape[1], fr.shape[2], C.c_void_p(out.data_ptr()),
                                                      out.stride(0), _lib.stream_ptr(), C.byref(bad)))
        if bad.value < 0:
            return None
        if bad.value < 3:
            return 'conv1+bn1+relu+maxpool'
        fused = None
        try:                                      # names of the unfused plan
            self.set_fusion(False)
            names = self.op_names()
        finally:
            self.set_fusion(True)
        return names[bad.value - 3] if bad.value - 3 < len(names) else 'launch %d' % bad.value

    def set_crop(self, pos):
        """0 = centre crop (reference), 1..4 = tl / tr / bl / br corner windows (pvr_encoder_set_crop_position)"""
        if self._handle is None:
            self._build()
        _lib.check(_lib.lib().pvr_encoder_set_crop_position(self._handle, int(pos)))

    def set_low_latency(self, on=True):
        """split-K plan for forwards of <= 4 frames (pvr_encoder_set_low_latency): the online EmbeddingWrapper pattern"""
        self._low_latency = bool(on)
        if self._handle is not None and not (self._clip or self._mae or self.variant == 'random5'):
            _lib.check(_lib.lib().pvr_encoder_set_low_latency(self._handle, int(self._low_latency)))

    def set_fusion(self, on):
        """A/B switch between the fused layer1/layer2 bottleneck-tail plan (default) and one launch per convolution;
        both give bit-identical outputs."""
        if self._handle is None:
            self._build()
        _lib.check(_lib.lib().pvr_encoder_debug_set_fusion(self._handle, 1 if on else 0))

    def tap(self, name, n_elems):
        """fp32 copy of an intermediate activation of the last forward (parity debugging)."""
        buf = torch.empty(n_elems, dtype=torch.float32, device='cuda')
        cnt = C.c_int64()
        _lib.check(_lib.lib().pvr_encoder_tap(self._handle, name.encode(), C.c_void_p(buf.data_ptr()), n_elems,
                                              C.byref(cnt), _lib.stream_ptr()))
        return buf[:cnt.value]

    def debug_stop_after(self, name):
        if self._handle is None:
            self._build()
        _lib.check(_lib.lib().pvr_encoder_debug_stop_after(self._handle, name.encode() if name else None))

    def forward(self, frames_u8):
        out = torch.empty((frames_u8.shape[0], self.out_size), dtype=torch.float32, device=frames_u8.device)
        self.forward_into(frames_u8, out)
        return out


_TRAINABLE = ('r18', 'r34', 'conv5')
_TRAINABLE_MSG = ("trainable (train=True) are the torchvision ResNet trunks: 'resnet18', 'resnet34', 'resnet50' and the conv5 checkpoints of the "
                  "registry (resnet50_places, demy, moco_*), in fp32 on one GPU")


class _EncoderFunction(torch.autograd.Function):
    """Training-mode forward of the whole encoder as one autograd node (the pattern of models._PolicyFunction).  Inputs: the module, the uint8
    frames, then every trained parameter (all, or those from train_from's stage up), so autograd routes a gradient to each of them.  The library keeps the activations of ONE forward: a backward
    after a later training forward of the same module raises.  The node keeps the uint8 frames (tiny next to an activation): with frozen BatchNorm
    a forward of more than max_batch frames ran as several passes, and the backward recomputes every pass but the last."""

    @staticmethod
    def forward(ctx, model, frames_u8, *params):
        out = model._forward_raw(frames_u8)
        model._fwd_gen += 1
        ctx.model, ctx.gen, ctx.frames = model, model._fwd_gen, frames_u8
        ctx.boundary, model._boundary = model._boundary, None       # (prefix_once: the cache lives on the node, exactly as long as the frames do)
        ctx.windows, model._windows = model._windows, None          # (random_crop: the step's windows, for the recompute passes that run the stem again)
        ctx.color, model._color = model._color, None                # (color_jitter: the step's parameters, parked and handed on exactly as the windows are)
        ctx.blur, model._blur = model._blur, None                   # (gaussian_blur / random_grayscale: likewise)
        return out

    @staticmethod
    def backward(ctx, dout):
        m = ctx.model
        if ctx.gen != m._fwd_gen:
            raise RuntimeError('trainable encoder backward: the activations of this forward are gone - a later training-mode forward of the same '
                               'encoder overwrote them (one backward per forward, right after it)')
        dout = dout.contiguous().float()
        g = torch.empty_like(m._flat)
        m._backward_raw(ctx.frames, dout, g, ctx.boundary, ctx.windows, ctx.color, ctx.blur)
        ctx.frames = ctx.boundary = ctx.windows = ctx.color = ctx.blur = None
        return (None, None) + tuple(g[o:o + n].view(shp) for o, n, shp in m._trained_slots)


class _CachedEncoderFunction(torch.autograd.Function):
    """_EncoderFunction on rows of a PrefixCache instead of uint8 frames (HipTrainableResNet.forward_cached): the node keeps the cache and the int64
    rows (tiny), the backward gathers every recomputed pass's rows again.  Inputs: the module, the cache, the rows, then the trained parameters only."""

    @staticmethod
    def forward(ctx, model, cache, rows, *params):
        out = model._forward_raw_cached(cache, rows)
        model._fwd_gen += 1
        ctx.model, ctx.gen, ctx.cache, ctx.rows = model, model._fwd_gen, cache, rows
        return out

    @staticmethod
    def backward(ctx, dout):
        m = ctx.model
        if ctx.gen != m._fwd_gen:
            raise RuntimeError('trainable encoder backward: the activations of this forward are gone - a later training-mode forward of the same '
                               'encoder overwrote them (one backward per forward, right after it)')
        dout = dout.contiguous().float()
        g = torch.empty_like(m._flat)
        m._backward_raw_cached(ctx.cache, ctx.rows, dout, g)
        ctx.cache = ctx.rows = None
        return (None, None, None) + tuple(g[o:o + n].view(shp) for o, n, shp in m._trained_slots)


class PrefixCache(object):
    """The boundary tensor of every frame of a dataset (HipTrainableResNet.build_prefix_cache): `data` is ONE (n_frames, boundary_floats) fp32 device
    tensor, row i what the frozen prefix gives for frame i.  It belongs to the encoder that built it, at that encoder's train_from stage, and is valid as
    long as that encoder's prefix has not been written: it records the encoder's prefix generation at build time (load_state_dict and
    invalidate_prefix_cache bump it) and a stale cache is refused, never used.  The trained parameters moving invalidates nothing."""

    def __init__(self, data, encoder, fill_seconds=0.0):
        self.data = data
        self.train_from = encoder.train_from
        self.generation = encoder._prefix_gen
        self.fill_seconds = float(fill_seconds)
        self._encoder = weakref.ref(encoder)

    @property
    def encoder(self):
        return self._encoder()

    @property
    def n_frames(self):
        return int(self.data.shape[0])

    @property
    def nbytes(self):
        return int(self.data.numel()) * 4


class HipTrainableResNet(_Node):
    """One trainable encoder (reference src/embeddings.py:323-326, :396-398): resnet18 / resnet34 / resnet50 in fp32 on the library's pvr_trainer
    (include/pvr_train.h).  Parameters are nn.Parameter CUDA views of ONE flat fp32 buffer the library reads on every forward, so any torch
    optimizer steps them in place; the BatchNorm buffers are views of a second block the training forward updates.  The tensors sit in the same
    _Node tree as HipResNet50's: state_dict() keys and shapes equal the frozen model's and the reference's.  In eval mode the module runs the
    frozen 'f32' plan (HipResNet50) built from the CURRENT parameters and running statistics.

    max_batch is the largest training batch: the workspace keeps the pre-BN, post-BN and gradient tensor of EVERY convolution for that many frames
    (about 0.03 GB per frame for resnet18 and 0.14 GB per frame for resnet50), so it defaults to 32, not to the frozen encoder's 256 - size it to
    the training batch.

    freeze_bn: frozen BatchNorm, the usual way to fine-tune a pre-trained trunk (torch: model.train() followed by .eval() on every BatchNorm
    module) - the convolutions and the BatchNorm affine parameters train, BatchNorm normalises with its running statistics and leaves them and
    num_batches_tracked untouched (pvr_trainer_set_bn_frozen).  Every frame is then independent of the others and max_batch is the CHUNK: a
    training-mode forward of n > max_batch frames runs as ceil(n / max_batch) passes in frame order, its backward recomputes each pass but the
    last (whose activations are still held) and accumulates the gradients (pvr_trainer_backward_acc: the last pass first, then the others in frame
    order), so the workspace is sized by the chunk and not by n.  n <= max_batch stays one forward and one backward.

    wgrad_split16: every weight gradient, conv1's included, as an exact-split product on the f16 matrix pipe (pvr_trainer_set_wgrad_split16: per-tensor
    power-of-two scales, three MFMAs per fragment pair, fp32 accumulation).  The forward, the data gradients and BatchNorm are untouched; a
    convolution weight gradient moves by about 2^-22 relative.  Chosen at construction (it decides the workspace); legal in both BatchNorm modes.

    conv_split16: every forward convolution and data gradient of layer1 .. layer4 as the same kind of product (pvr_trainer_set_conv_split16: both
    operands scaled per tensor on the device, so gradients of 1e-6 and activations past 65504 keep their precision); conv1's forward, BatchNorm, the
    pools and - unless wgrad_split16 is on as well - the weight gradients stay fp32.  Embeddings and gradients move by about 2^-22 relative per
    product.  Chosen at construction; legal in both BatchNorm modes, with or without wgrad_split16.  Eval mode keeps running the frozen 'f32' plan.

    train_from: None (everything trains) or 'layer1' .. 'layer4' - partial fine-tuning (pvr_trainer_set_train_from): that stage and the ones above it
    train; conv1 / bn1 and the stages below are the frozen prefix (torch: those modules in .eval() with requires_grad = False).  The prefix runs on its
    running statistics in either BatchNorm mode, keeps no activation but the one the first trained block reads, and has no backward: the workspace
    (workspace_bytes) and the step shrink with the stage.  Prefix parameters stay nn.Parameters with requires_grad = False and stay in state_dict();
    the autograd node takes only the trained parameters, so a prefix parameter's .grad stays None.  Chosen at construction (it decides the
    workspace); legal in both BatchNorm modes and with either or both split modes.

    prefix_once (needs train_from): the frozen prefix runs once per frame and step.  A training forward allocates one (n, boundary_floats) fp32 tensor -
    the one prefix tensor a trained op reads, trainer_boundary_bytes per frame - every pass writes its rows (pvr_trainer_forward_boundary), and the
    recompute passes of a chunked backward start at the first trained op on theirs instead of running preprocess, the stem and the prefix again.  The
    tensor lives as long as the kept uint8 frames do and is released after the backward.  With conv_split16 a prefix op is also one launch instead of
    three (pvr_trainer_set_prefix_fused), and the workspace holds no pre-BN tensor of the prefix.  Embeddings and gradients keep their bits.  Chosen at
    construction; legal in both BatchNorm modes (with batch statistics a step is one pass and only the fused launches matter) and with either split mode.

    prefix_cache (needs train_from): the frozen prefix runs once per DATASET frame.  build_prefix_cache(frames) computes the boundary tensor of every
    frame once, before training, into a PrefixCache (pvr_trainer_prefix_forward in blocks of max_batch); forward_cached(cache, rows) is then the
    training forward of the frames behind those cache rows: every pass gathers its rows into ONE staging tensor of max_batch x boundary_floats
    (pvr_op_gather_rows) and starts at the first trained op (pvr_trainer_forward_boundary with reuse), in the forward and in the recompute passes of
    the backward.  No uint8 frame is touched.  The keyword only selects the workspace mode (the fused prefix launches of prefix_once, so that the
    cache's bits are that mode's); together with prefix_once it means prefix_cache and no step-sized boundary tensor is allocated.  Embeddings and
    gradients keep the bits of a step on the frames themselves, with prefix_once and with neither mode.

    random_crop: a random crop window per frame and step, the augmentation of fine-tuning on few small frames.  In training mode every frame of a forward
    goes through Resize(256) and then its OWN 224 x 224 window of the resized frame instead of the centre one: the step's (n, 2) int32 windows (top, left)
    are drawn once on the device (pvr_op_crop_windows with seed = crop_seed, call = crop_call, first_frame = 0: frame i of the forward is frame i of the
    draw, so the two frames of an observation get independent windows), every pass is handed its rows (pvr_trainer_forward_windows: one launch writes the
    windowed fp32 image) and so is every recompute pass of a chunked backward that runs the stem again, so it sees the same image; with prefix_once the
    recompute passes start at the boundary tensor as without the mode.  crop_call, a plain int attribute, then goes up by one: a caller that sets it
    (the driver: the iteration's number) makes a resumed run draw what an uninterrupted one would, and crop_windows(crop_seed, call, n, max_top,
    max_left) predicts a step's windows on the host.  Off by default; with it off nothing moves.  Eval mode keeps the centre crop on the frozen 'f32'
    plan.  Not with prefix_cache, build_prefix_cache or forward_cached: a cache holds the prefix's output for ONE window per frame.

    color_jitter: brightness, contrast and saturation per frame and step - torchvision's ColorJitter on the uint8 values of the frame's 224 x 224 window,
    after Resize and the window and before / 255 and Normalize, where T.ColorJitter would sit in the reference's transforms.  (b, c, s) are the three
    strengths, a scalar means all three, None or zeros mean off: a factor is uniform in [max(0, 1 - strength), 1 + strength], and every frame gets its own
    random order of the three ops.  Hue is not offered.  In training mode the step's (n, 4) parameters (float b, c, s and the int32 order code,
    include/pvr_train.h) are drawn once on the device (pvr_op_color_params with seed = color_seed and call = crop_call, the SAME per-forward counter
    random_crop uses, which goes up by one per training forward whenever either mode is on); every pass is handed its rows
    (pvr_trainer_forward_augmented: the launches "colour stats" and "preprocess colour" write the jittered fp32 image), and so is every recompute pass
    that runs the stem again.  Without random_crop every frame's window is the centre one.  color_params(color_seed, call, n, strengths) predicts a
    step's parameters on the host.  Off by default; with it off nothing moves, and random_crop's windows keep their bits with it on.  Eval mode keeps
    the un-jittered centre crop.  Not with prefix_cache, build_prefix_cache or forward_cached: a cache holds the prefix's output for ONE image per frame;
    prefix_once is the compatible mode.

    random_resized_crop: torchvision's RandomResizedCrop(224, scale=(lo, hi), ratio=(3/4, 4/3)) per frame and step - the crop MoCo's checkpoints were
    pre-trained with: a rectangle of random area (uniform in [lo, hi] of the frame's) and aspect ratio (log-uniform in [3/4, 4/3]) of the ORIGINAL uint8
    frame, resized to 224 x 224.  It takes the place of Resize(256) plus the window and sits before color_jitter, / 255 and Normalize.  (lo, hi) is the
    scale range, a scalar s means (s, 1.0), None is off.  In training mode the step's (n, 4) rectangles (top, left, height, width; include/pvr_train.h)
    are drawn once on the device (pvr_op_crop_rects with seed = crop_seed and call = crop_call, the per-forward counter of the other two modes); every pass
    is handed its rows (pvr_trainer_forward_rects: the launch "preprocess rects", or with color_jitter the colour pair reading the rectangle, writes the
    fp32 image), and so is every recompute pass that runs the stem again - the rectangles are parked where random_crop's windows are.  crop_rects(
    crop_seed, call, n, h, w, scale) predicts a step's rectangles on the host.  A frame smaller than the crop is legal (no Resize runs).  Off by default;
    with it off nothing moves.  Eval mode keeps Resize(256) and the centre crop.  Not with random_crop (both choose the window), and not with prefix_cache,
    build_prefix_cache or forward_cached; it composes with color_jitter, prefix_once, frozen BatchNorm chunking and the split modes.

    gaussian_blur, random_grayscale: the last two augmentations of MoCo v2's recipe, per frame and step.  gaussian_blur=(p, lo, hi): with probability p a
    frame is blurred as torchvision's GaussianBlur(kernel_size=23, sigma=(lo, hi)) blurs a uint8 tensor, sigma uniform in [lo, hi] (MoCo v2: (0.5, 0.1,
    2.0); the kernel size is fixed at 23, PIL's radius semantics are not offered).  random_grayscale=p: with probability p the three channels of a frame
    become its gray value, torchvision's rgb_to_grayscale(num_output_channels=3) on uint8 (MoCo v2: 0.2).  None or a probability of 0: off.  Order per
    frame: window or rectangle, colour jitter, grayscale, blur, / 255, Normalize.  In training mode the step's (n, 2) parameters (float sigma, 0 for not
    blurred, and int32 gray; include/pvr_train.h) are drawn once on the device (pvr_op_blur_params with seed = blur_seed and call = crop_call) and parked
    as the colour parameters are; every pass is handed its rows (pvr_trainer_forward_staged: the launches "stage image" - the uint8 image into a staging
    buffer of max_batch x 224 x 224 x 4 bytes, made once next to the gray sums - and "blur normalize" stand where the image launch stood), and so is
    every recompute pass that runs the stem again.  blur_params(blur_seed, call, n, gaussian_blur, random_grayscale) predicts a step's parameters on the
    host.  Off by default; with both off nothing moves, and the windows, rectangles and colour parameters keep their bits with them on.  Eval mode keeps
    the plain centre crop.  Not with prefix_cache, build_prefix_cache or forward_cached; they compose with each other, random_crop or
    random_resized_crop, color_jitter, prefix_once, frozen BatchNorm chunking, train_from and the split modes."""

    def __init__(self, state_dict, variant='conv5', max_batch=None, freeze_bn=False, wgrad_split16=False, conv_split16=False, train_from=None,
                 prefix_once=False, prefix_cache=False, random_crop=False, crop_seed=0, color_jitter=None, color_seed=0,
                 random_resized_crop=None, gaussian_blur=None, random_grayscale=None, blur_seed=0):
        super().__init__()
        assert variant in _TRAINABLE, variant
        blur, gray = blur_spec(gaussian_blur), gray_prob(random_grayscale)
        check_gaussian_blur(blur, gray, prefix_cache)
        check_random_crop(random_crop, prefix_cache)
        rrc_scale = crop_scale(random_resized_crop)
        check_random_resized_crop(rrc_scale, prefix_cache, random_crop=random_crop)
        strengths = color_strengths(color_jitter)
        check_color_jitter(strengths, prefix_cache)
        _lib.require_gpu()
        self.variant = variant
        self.out_size = OUT_SIZE[variant]
        self._dtype = _lib.PVR_F32
        self._max_batch = int(max_batch or 32)
        self._fwd_gen = 0
        self._freeze_bn = False
        self._acc_scratch = None                 # one pass's gradient (a chunked backward only), made on first use
        self._frozen = []                        # the eval-mode plan, in a plain list: not a sub-module (its tensors are no part of state_dict())
        L = _lib.lib()
        tr = transforms_for('')
        desc = _lib.EncoderDesc(arch=_ARCH[variant], dtype=_lib.PVR_F32, max_batch=self._max_batch, chunk=0, resize=tr.resize, crop=tr.crop)
        desc.mean[:] = tr.mean
        desc.std_[:] = tr.std
        h = C.c_void_p()
        _lib.check(L.pvr_trainer_create(C.byref(desc), C.byref(h)))
        self._handle = h
        self._wgrad_split16 = False
        if wgrad_split16:
            self.set_wgrad_split16(True)
        self._conv_split16 = False
        if conv_split16:
            self.set_conv_split16(True)
        self._train_from = None
        if train_stage(train_from):
            _lib.check(L.pvr_trainer_set_train_from(h, train_stage(train_from)))
            self._train_from = train_from
        check_prefix_once(prefix_once, train_from)
        check_prefix_cache(prefix_cache, train_from)
        self._prefix_cache = bool(prefix_cache)
        self._prefix_gen = 0                     # bumped by every write path to the frozen prefix: a PrefixCache of an older generation is refused
        self._staging = None                     # prefix_cache: the (max_batch, boundary_floats) tensor a cached pass gathers its rows into, made once
        self._prefix_once = bool(prefix_once) and not self._prefix_cache      # (both: prefix_cache - no step-sized boundary tensor)
        self._boundary = None                    # prefix_once: the boundary cache between _forward_raw and its consumer (the autograd node or the joint step)
        self._boundary_floats = int(L.pvr_trainer_boundary_floats(h))
        self._random_crop = bool(random_crop)
        self.crop_seed = int(crop_seed)          # random_crop: Philox key of the windows
        self.crop_call = 0                       # random_crop: the next training forward's draw; it goes up by one per forward and a caller may set it
        self._windows = None                     # random_crop: the step's windows between _forward_raw and its consumer (parked as _boundary is)
        self._rrc_scale = rrc_scale              # random_resized_crop: the (lo, hi) share of the frame's area, None when off (seed and call: crop_seed, crop_call)
        self._color_jitter = strengths           # color_jitter: the three strengths, None when off
        self.color_seed = int(color_seed)        # color_jitter: Philox key of the parameters (the call number is crop_call)
        self._color = None                       # color_jitter: the step's parameters between _forward_raw and its consumer (parked as _windows is)
        self._gray_sums = None                   # color_jitter: max_batch uint32 of scratch for a pass's gray sums (the trainer's workspace holds none)
        self._gaussian_blur = blur               # gaussian_blur: (p, sigma lo, sigma hi), None when off
        self._random_grayscale = gray            # random_grayscale: the probability, None when off
        self.blur_seed = int(blur_seed)          # gaussian_blur / random_grayscale: Philox key of the parameters (the call number is crop_call)
        self._blur = None                        # the step's (n, 2) blur parameters between _forward_raw and its consumer (parked as _color is)
        self._staged = None                      # max_batch x crop x crop x 4 bytes of scratch for a pass's staged uint8 image (made once, as _gray_sums is)
        self._resize, self._crop = int(tr.resize), int(tr.crop)
        if self._prefix_once or self._prefix_cache:
            _lib.check(L.pvr_trainer_set_prefix_fused(h, 1))
        self._trained_offset = int(L.pvr_trainer_trained_offset(h))     # floats of the flat buffer below it are the frozen prefix (one leading span)
        dev = torch.device('cuda')
        self._flat = torch.zeros(L.pvr_trainer_param_count(h), dtype=torch.float32, device=dev)
        self._bufs = torch.zeros(L.pvr_trainer_buffer_count(h), dtype=torch.float32, device=dev)
        self._slots = []                         # (offset, numel, shape) of every parameter, in the order they are handed to autograd
        self._plist = []
        numel, shape = C.c_int64(), (C.c_int64 * 4)()
        for k, v in state_dict.items():
            t = (v if isinstance(v, torch.Tensor) else torch.from_numpy(np.asarray(v))).detach()
            if k.endswith(('running_mean', 'running_var', 'num_batches_tracked')):
                o = L.pvr_trainer_buffer_offset(h, k.encode(), C.byref(numel))
                if o < 0:
                    raise KeyError("trainable '%s' encoder: unexpected state_dict key %r" % (variant, k))
                if k.endswith('num_batches_tracked'):
                    view = self._bufs[o:o + 2].view(torch.int64).view(())
                else:
                    view = self._bufs[o:o + numel.value]
                view.copy_(t.to(device=dev, dtype=view.dtype).reshape(view.shape))
                _install(self, k, view)
            else:
                o = L.pvr_trainer_param_offset(h, k.encode(), C.byref(numel), shape)
                if o < 0:
                    raise KeyError("trainable '%s' encoder: unexpected state_dict key %r" % (variant, k))
                shp = tuple(int(x) for x in shape if x > 0)
                assert tuple(t.shape) == shp, (k, tuple(t.shape), shp)
                view = self._flat[o:o + numel.value].view(shp)
                view.copy_(t.to(device=dev, dtype=torch.float32))
                _install(self, k, view)
                self._slots.append((o, numel.value, shp))
                self._plist.append(self.get_parameter(k))
        missing = sum(n for _, n, _ in self._slots) != self._flat.numel()
        if missing:                               # (the reference asserts missing_keys == [], moco.py:24)
            raise KeyError("trainable '%s' encoder: the state_dict does not hold every parameter" % variant)
        trained = [i for i, (o, _, _) in enumerate(self._slots) if o >= self._trained_offset]
        self._trained_slots = [self._slots[i] for i in trained]
        self._trained_plist = [self._plist[i] for i in trained]
        if freeze_bn:
            self.set_bn_frozen(True)

    # -- lifetime ------------------------------------------------------------------------------
    def close(self):
        """free the frozen eval-mode plan now; the trainer handle lives as long as the module (its parameters are views the library reads)"""
        for m in self._frozen:
            m.close()
        del self._frozen[:]

    def __del__(self):
        try:
            self.close()
            if self._handle is not None:
                _lib.lib().pvr_trainer_destroy(self._handle)
                self._handle = None
        except Exception:
            pass

    def train(self, mode=True):
        self.close()                              # the frozen plan folds the parameters of the moment it is built
        return super().train(mode)

    def load_state_dict(self, *a, **k):
        self.close()
        self.invalidate_prefix_cache()
        return super().load_state_dict(*a, **k)

    def _load_from_state_dict(self, *a, **k):
        self.invalidate_prefix_cache()            # (a parent module's load_state_dict comes through here, not through load_state_dict above)
        return super()._load_from_state_dict(*a, **k)

    def invalidate_prefix_cache(self):
        """a parameter or buffer of the frozen prefix may have moved: every PrefixCache built before this call is refused from now on.  load_state_dict
        calls it; so must whoever writes a prefix tensor in place"""
        self._prefix_gen += 1

    @property
    def max_batch(self):
        return self._max_batch

    @property
    def freeze_bn(self):
        return self._freeze_bn

    def set_bn_frozen(self, on=True):
        """frozen BatchNorm on / off (see the class docstring); a training forward still waiting for its backward loses its activations"""
        _lib.check(_lib.lib().pvr_trainer_set_bn_frozen(self._handle, 1 if on else 0))
        self._freeze_bn = bool(on)
        self._fwd_gen += 1

    @property
    def train_from(self):
        """None or 'layer1' .. 'layer4' (see the class docstring)"""
        return self._train_from

    @property
    def prefix_once(self):
        """the frozen prefix runs once per frame and step (see the class docstring)"""
        return self._prefix_once

    def boundary_bytes(self):
        """bytes per frame of the boundary tensor prefix_once keeps (0 when everything trains)"""
        return 4 * self._boundary_floats

    @property
    def random_crop(self):
        """a training forward crops a random window per frame (see the class docstring)"""
        return self._random_crop

    @property
    def random_resized_crop(self):
        """the (lo, hi) scale range of a training forward's random resized crop, None when off (see the class docstring)"""
        return self._rrc_scale

    @property
    def gaussian_blur(self):
        """the (p, sigma lo, sigma hi) of a training forward's Gaussian blur, None when off (see the class docstring)"""
        return self._gaussian_blur

    @property
    def random_grayscale(self):
        """the probability of a training forward's grayscale, None when off (see the class docstring)"""
        return self._random_grayscale

    @property
    def color_jitter(self):
        """the (brightness, contrast, saturation) strengths of a training forward's colour jitter, None when off (see the class docstring)"""
        return self._color_jitter

    def crop_range(self, h, w):
        """(max_top, max_left) of an (h, w) frame's window: its size after Resize minus the crop (32, 32 for square frames)"""
        rh, rw = resized_size(h, w, self._resize)
        if rh < self._crop or rw < self._crop:
            raise ValueError('random_crop: a %dx%d frame is %dx%d after Resize(%d), smaller than the %d crop' % (h, w, rh, rw, self._resize, self._crop))
        return rh - self._crop, rw - self._crop

    @property
    def prefix_cache(self):
        """the workspace was made for cached steps (see the class docstring)"""
        return self._prefix_cache

    def build_prefix_cache(self, frames_u8):
        """(N, H, W, 3) uint8 device frames -> a PrefixCache of their N boundary tensors, filled in blocks of max_batch by pvr_trainer_prefix_forward.
        Always switches the fused prefix launches on (prefix_once's workspace mode): call it before the first training forward, or on an encoder
        constructed with prefix_cache=True or prefix_once=True - once the workspace exists without that mode the library refuses with a state error.
        A training forward still waiting for its backward loses its activations."""
        if self._train_from is None:
            raise ValueError('build_prefix_cache needs train_from: with everything training there is no frozen prefix whose output could be cached')
        check_random_crop(self._random_crop, True, 'build_prefix_cache')
        check_color_jitter(self._color_jitter, True, 'build_prefix_cache')
        check_random_resized_crop(self._rrc_scale, True, 'build_prefix_cache')
        check_gaussian_blur(self._gaussian_blur, self._random_grayscale, True, 'build_prefix_cache')
        return self._build_prefix_cache(int(frames_u8.shape[0]), [(0, frames_u8)])

    def _build_prefix_cache(self, n_frames, blocks):
        """build_prefix_cache from an iterable of (first cache row, (k, H, W, 3) uint8 device frames) blocks that cover [0, n_frames): a caller whose
        frames are not laid out as one (N, H, W, 3) tensor (PolicyNetWithEncoder: F frames side by side per sample) splits block by block"""
        if self._train_from is None:
            raise ValueError('build_prefix_cache needs train_from: with everything training there is no frozen prefix whose output could be cached')
        check_random_crop(self._random_crop, True, 'build_prefix_cache')
        check_color_jitter(self._color_jitter, True, 'build_prefix_cache')
        check_random_resized_crop(self._rrc_scale, True, 'build_prefix_cache')
        check_gaussian_blur(self._gaussian_blur, self._random_grayscale, True, 'build_prefix_cache')
        L = _lib.lib()
        _lib.check(L.pvr_trainer_set_prefix_fused(self._handle, 1))
        vp = lambda t: C.c_void_p(t.data_ptr())
        data = torch.empty((n_frames, self._boundary_floats), dtype=torch.float32, device=self._flat.device)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        self._fwd_gen += 1                        # (the stem's workspace is overwritten: a held forward is gone)
        filled = 0
        for row0, frames_u8 in blocks:
            n, h, w, c = frames_u8.shape
            assert c == 3 and frames_u8.dtype == torch.uint8 and frames_u8.is_cuda and frames_u8.is_contiguous() and row0 == filled and row0 + n <= n_frames
            for lo in range(0, n, self._max_batch):
                hi = min(lo + self._max_batch, n)
                _lib.check(L.pvr_trainer_prefix_forward(self._handle, vp(self._flat), vp(self._bufs), vp(frames_u8[lo:hi]), hi - lo, h, w,
                                                        vp(data[row0 + lo:row0 + hi]), _lib.stream_ptr()))
            filled += n
        assert filled == n_frames, (filled, n_frames)
        torch.cuda.synchronize()
        return PrefixCache(data, self, time.perf_counter() - t0)

    def check_prefix_cache(self, cache):
        """raise unless `cache` is a PrefixCache this encoder may use now: of this stage, of this encoder, of the current prefix generation"""
        if not isinstance(cache, PrefixCache):
            raise TypeError('forward_cached takes a PrefixCache (build_prefix_cache), got %s' % type(cache).__name__)
        if cache.train_from != self._train_from:
            raise RuntimeError('prefix cache of another stage: it holds the boundary tensors of train_from %r, this encoder trains from %r'
                               % (cache.train_from, self._train_from))
        if cache.encoder is not self or cache.data.shape[1] != self._boundary_floats:
            raise RuntimeError('prefix cache of another encoder: a cache holds what the frozen prefix of the encoder that built it computes; build one '
                               'with this encoder\'s build_prefix_cache')
        if cache.generation != self._prefix_gen:
            raise RuntimeError('stale prefix cache: the encoder\'s frozen prefix may have been written since the cache was built (load_state_dict or '
                               'invalidate_prefix_cache; generation %d, the cache has %d): rebuild it with build_prefix_cache'
                               % (self._prefix_gen, cache.generation))

    def forward_cached(self, cache, rows):
        """training-mode forward of the frames behind `rows` (int64 device tensor, one row of `cache` per frame): embeddings with a graph that hands
        only the trained parameters to autograd.  The bits of forward(frames[rows])."""
        check_random_crop(self._random_crop, True, 'forward_cached')
        check_color_jitter(self._color_jitter, True, 'forward_cached')
        check_random_resized_crop(self._rrc_scale, True, 'forward_cached')
        check_gaussian_blur(self._gaussian_blur, self._random_grayscale, True, 'forward_cached')
        self.check_prefix_cache(cache)
        if not self.training:
            raise RuntimeError('forward_cached is a training-mode forward (the cache holds the input of the trained stages): in eval mode embed the '
                               'frames themselves')
        self.close()
        return _CachedEncoderFunction.apply(self, cache, self._cache_rows(cache, rows), *self._trained_plist)

    def _cache_rows(self, cache, rows):
        if not (isinstance(rows, torch.Tensor) and rows.dtype == torch.int64 and rows.device == cache.data.device):
            raise TypeError('forward_cached: rows is an int64 tensor on the cache\'s device, one cache row per frame')
        return rows.reshape(-1).contiguous()

    @property
    def trained_offset(self):
        """float offset in the flat parameter buffer at which the trained parameters begin (pvr_trainer_trained_offset; 0 when everything trains)"""
        return self._trained_offset

    def trained_parameters(self):
        """the parameters a training step moves: all of them, or those of train_from's stage and above"""
        return list(self._trained_plist)

    def prefix_parameters(self):
        """the parameters of the frozen prefix (empty unless train_from is set)"""
        t = set(id(p) for p in self._trained_plist)
        return [p for p in self._plist if id(p) not in t]

    @property
    def wgrad_split16(self):
        return self._wgrad_split16

    def set_wgrad_split16(self, on=True):
        """split-f16 weight gradients on / off (see the class docstring); only before the first training forward has made the workspace - afterwards
        the library refuses with a state error"""
        _lib.check(_lib.lib().pvr_trainer_set_wgrad_split16(self._handle, 1 if on else 0))
        self._wgrad_split16 = bool(on)

    @property
    def conv_split16(self):
        return self._conv_split16

    def set_conv_split16(self, on=True):
        """split-f16 forward convolutions and data gradients on / off (see the class docstring); only before the first training forward has made the
        workspace - afterwards the library refuses with a state error"""
        _lib.check(_lib.lib().pvr_trainer_set_conv_split16(self._handle, 1 if on else 0))
        self._conv_split16 = bool(on)

    def _passes(self, n):
        """[(lo, hi)] of the passes of a training forward of n frames, in frame order"""
        return [(lo, min(lo + self._max_batch, n)) for lo in range(0, n, self._max_batch)]

    def workspace_bytes(self):
        """device bytes of the training workspace the first forward allocates for max_batch frames (pvr_trainer_workspace_bytes)"""
        return int(_lib.lib().pvr_trainer_workspace_bytes(self._handle))

    @property
    def lanes(self):
        return 4

    def set_low_latency(self, on=True):
        self._low_latency = bool(on)

    def _eval_model(self):
        if not self._frozen:
            self._frozen.append(HipResNet50({k: v.detach().cpu() for k, v in self.state_dict().items()}, self.variant, compute_dtype='f32',
                                            max_batch=self._max_batch))
            if getattr(self, '_low_latency', False):
                self._frozen[0].set_low_latency(True)
        return self._frozen[0]

    def forward_into(self, frames_u8, out, lane=0):
        """eval mode only (the streaming embedders): the frozen 'f32' plan of the current parameters"""
        if self.training:
            raise RuntimeError('forward_into is the frozen encoder\'s entry point: call .eval() first (a training-mode forward returns a tensor with a graph)')
        self._eval_model().forward_into(frames_u8, out, lane=lane)

    def _forward_raw(self, frames_u8):
        n, h, w, c = frames_u8.shape
        assert c == 3 and frames_u8.dtype == torch.uint8 and frames_u8.is_cuda and frames_u8.is_contiguous()
        if n > self._max_batch and not self._freeze_bn:
            raise ValueError('training forward of %d frames: the workspace was made for max_batch = %d (BatchNorm takes the whole batch together, '
                             'it cannot be chunked)' % (n, self._max_batch))
        out = torch.empty((n, self.out_size), dtype=torch.float32, device=frames_u8.device)
        # prefix_once: the boundary tensor of every frame of the step; its consumer (the autograd node, or the joint step under the generation
        # counter) takes it from here and hands it to _backward_raw
        self._boundary = torch.empty((n, self._boundary_floats), dtype=torch.float32, device=frames_u8.device) if self._prefix_once else None
        # random_crop: the step's windows, drawn once; every pass takes its rows, and the consumer hands the tensor to _backward_raw like the boundary cache
        self._windows = None
        if self._random_crop:
            max_top, max_left = self.crop_range(h, w)
            self._windows = torch.empty((n, 2), dtype=torch.int32, device=frames_u8.device)
            _lib.check(_lib.lib().pvr_op_crop_windows(self.crop_seed, self.crop_call, 0, n, max_top, max_left, C.c_void_p(self._windows.data_ptr()),
                                                      _lib.stream_ptr()))
        # random_resized_crop: the step's rectangles (n, 4) of the original frames, drawn once under the same call number and parked in the windows' place
        # (the two modes exclude each other): every consumer hands _windows on as it is, and a pass tells the two by the row length
        if self._rrc_scale is not None:
            self._windows = torch.empty((n, 4), dtype=torch.int32, device=frames_u8.device)
            _lib.check(_lib.lib().pvr_op_crop_rects(self.crop_seed, self.crop_call, 0, n, h, w, self._rrc_scale[0], self._rrc_scale[1],
                                                    C.c_void_p(self._windows.data_ptr()), _lib.stream_ptr()))
        # color_jitter: the step's parameters, drawn once under the same call number and parked the same way; without random_crop every frame's window
        # is the centre one
        self._color = None
        if self._color_jitter is not None:
            if self._windows is None:
                max_top, max_left = self.crop_range(h, w)
                self._windows = torch.tensor([int(round(max_top / 2.0)), int(round(max_left / 2.0))], dtype=torch.int32,
                                                 device=frames_u8.device).repeat(n, 1)
            self._color = torch.empty((n, 4), dtype=torch.int32, device=frames_u8.device)
            _lib.check(_lib.lib().pvr_op_color_params(self.color_seed, self.crop_call, 0, n, *self._color_jitter, C.c_void_p(self._color.data_ptr()),
                                                      _lib.stream_ptr()))
        # gaussian_blur / random_grayscale: the step's (n, 2) parameters, drawn once under the same call number and parked the same way; without a random
        # window every frame's window is the centre one
        self._blur = None
        if self._gaussian_blur is not None or self._random_grayscale is not None:
            if self._windows is None:
                max_top, max_left = self.crop_range(h, w)
                self._windows = torch.tensor([int(round(max_top / 2.0)), int(round(max_left / 2.0))], dtype=torch.int32,
                                             device=frames_u8.device).repeat(n, 1)
            self._blur = torch.empty((n, 2), dtype=torch.int32, device=frames_u8.device)
            _lib.check(_lib.lib().pvr_op_blur_params(self.blur_seed, self.crop_call, 0, n, *(self._gaussian_blur or (0.0, 1.0, 1.0)),
                                                     self._random_grayscale or 0.0, C.c_void_p(self._blur.data_ptr()), _lib.stream_ptr()))
        if self._random_crop or self._color_jitter is not None or self._rrc_scale is not None or self._blur is not None:
            self.crop_call += 1
        for lo, hi in self._passes(n):            # (one pass unless BatchNorm is frozen; the last pass's activations stay held)
            self._forward_pass(frames_u8, lo, hi, out[lo:hi], self._boundary, windows=self._windows, color=self._color, blur=self._blur)
        return out

    def _forward_pass(self, frames_u8, lo, hi, out, boundary=None, reuse=False, windows=None, color=None, blur=None):
        """one pass over frames [lo, hi).  boundary: the step's (n, boundary_floats) cache - this pass writes its rows (reuse False) or starts at the first
        trained op on what they hold (reuse True).  windows (random_crop): the step's (n, 2) int32 windows - this pass crops at its rows.  color
        (color_jitter, with windows): the step's (n, 4) parameters - this pass jitters its rows.  windows of four columns (random_resized_crop): the
        step's rectangles - this pass resizes each frame's own rectangle to the crop, with or without color.  blur (gaussian_blur / random_grayscale, with
        windows of either kind): the step's (n, 2) parameters - this pass stages its uint8 image and grays and blurs its rows"""
        vp = lambda t: C.c_void_p(t.data_ptr())
        if blur is not None:
            reuse = reuse and boundary is not None                            # (as below: without a boundary cache a recompute pass makes the same image again)
            if color is not None and self._gray_sums is None:
                self._gray_sums = torch.empty((self._max_batch,), dtype=torch.int32, device=blur.device)
            if self._staged is None:
                self._staged = torch.empty((self._max_batch, self._crop, self._crop, 4), dtype=torch.uint8, device=blur.device)
            rects = windows.shape[1] == 4
            _lib.check(_lib.lib().pvr_trainer_forward_staged(self._handle, vp(self._flat), vp(self._bufs), None if reuse else vp(frames_u8[lo:hi]), hi - lo,
                                                             frames_u8.shape[1], frames_u8.shape[2], None if rects else vp(windows[lo:hi]),
                                                             vp(windows[lo:hi]) if rects else None, None if color is None else vp(color[lo:hi]),
                                                             None if color is None else vp(self._gray_sums), vp(blur[lo:hi]), vp(self._staged),
                                                             None if boundary is None else vp(boundary[lo:hi]), 1 if reuse else 0, vp(out), out.stride(0),
                                                             _lib.stream_ptr()))
            return
        if windows is not None and windows.shape[1] == 4:
            reuse = reuse and boundary is not None                            # (as below: without a boundary cache a recompute pass makes the same image again)
            if color is not None and self._gray_sums is None:
                self._gray_sums = torch.empty((self._max_batch,), dtype=torch.int32, device=color.device)
            _lib.check(_lib.lib().pvr_trainer_forward_rects(self._handle, vp(self._flat), vp(self._bufs), None if reuse else vp(frames_u8[lo:hi]), hi - lo,
                                                            frames_u8.shape[1], frames_u8.shape[2], vp(windows[lo:hi]),
                                                            None if color is None else vp(color[lo:hi]),
                                                            None if color is None else vp(self._gray_sums),
                                                            None if boundary is None else vp(boundary[lo:hi]), 1 if reuse else 0, vp(out), out.stride(0),
                                                            _lib.stream_ptr()))
            return
        if color is not None:
            reuse = reuse and boundary is not None                            # (as below: without a boundary cache a recompute pass makes the same image again)
            if self._gray_sums is None:
                self._gray_sums = torch.empty((self._max_batch,), dtype=torch.int32, device=color.device)
            _lib.check(_lib.lib().pvr_trainer_forward_augmented(self._handle, vp(self._flat), vp(self._bufs), None if reuse else vp(frames_u8[lo:hi]), hi - lo,
                                                                frames_u8.shape[1], frames_u8.shape[2], vp(windows[lo:hi]), vp(color[lo:hi]),
                                                                vp(self._gray_sums), None if boundary is None else vp(boundary[lo:hi]),
                                                                1 if reuse else 0, vp(out), out.stride(0), _lib.stream_ptr()))
            return
        if windows is not None:
            reuse = reuse and boundary is not None                            # (without a boundary cache a recompute pass runs the stem again, at the same windows)
            _lib.check(_lib.lib().pvr_trainer_forward_windows(self._handle, vp(self._flat), vp(self._bufs), None if reuse else vp(frames_u8[lo:hi]), hi - lo,
                                                              frames_u8.shape[1], frames_u8.shape[2], vp(windows[lo:hi]),
                                                              None if boundary is None else vp(boundary[lo:hi]), 1 if reuse else 0, vp(out),
                                                              out.stride(0), _lib.stream_ptr()))
            return
        if boundary is None:
            _lib.check(_lib.lib().pvr_trainer_forward(self._handle, vp(self._flat), vp(self._bufs), vp(frames_u8[lo:hi]), hi - lo, frames_u8.shape[1],
                                                      frames_u8.shape[2], vp(out), out.stride(0), _lib.stream_ptr()))
            return
        h, w = (0, 0) if frames_u8 is None else frames_u8.shape[1:3]     # (a reuse pass reads no frames: forward_cached has none)
        _lib.check(_lib.lib().pvr_trainer_forward_boundary(self._handle, vp(self._flat), vp(self._bufs), None if reuse else vp(frames_u8[lo:hi]), hi - lo,
                                                           h, w, vp(boundary[lo:hi]), 1 if reuse else 0, vp(out),
                                                           out.stride(0), _lib.stream_ptr()))

    def _backward_raw(self, frames_u8, dout, grads, boundary=None, windows=None, color=None, blur=None):
        """d(loss)/d(embeddings) of the training forward that just ran on frames_u8 -> the flat gradient `grads` (fully written).  One pass: one
        pvr_trainer_backward.  Several (frozen BatchNorm): the last pass first - its activations are still held - then every other pass in frame
        order, each recomputed and added by pvr_trainer_backward_acc.  boundary (prefix_once): the cache that forward filled; a recomputed pass
        starts at the first trained op on its rows.  windows (random_crop): the windows that forward drew; a recomputed pass that runs the stem crops
        at its rows again (random_resized_crop: the rectangles, four columns, in the same place).  color (color_jitter): the parameters that forward
        drew, for the same passes; blur (gaussian_blur / random_grayscale): the blur parameters, likewise."""
        L = _lib.lib()
        vp = lambda t: C.c_void_p(t.data_ptr())
        passes = self._passes(frames_u8.shape[0])
        assert dout.shape[0] == frames_u8.shape[0] and dout.stride(1) == 1
        assert (boundary is not None) == self._prefix_once, 'prefix_once: the backward takes the boundary cache of its forward'
        staged = self._gaussian_blur is not None or self._random_grayscale is not None
        assert (windows is not None) == (self._random_crop or self._color_jitter is not None or self._rrc_scale is not None or staged), \
            'random_crop / color_jitter / random_resized_crop / gaussian_blur / random_grayscale: the backward takes the windows or rectangles of its forward'
        assert (blur is not None) == staged, 'gaussian_blur / random_grayscale: the backward takes the blur parameters of its forward'
        assert (color is not None) == (self._color_jitter is not None), 'color_jitter: the backward takes the colour parameters of its forward'
        if len(passes) == 1:
            _lib.check(L.pvr_trainer_backward(self._handle, vp(self._flat), vp(dout), dout.stride(0), vp(grads), _lib.stream_ptr()))
            return
        if self._acc_scratch is None:
            self._acc_scratch = torch.empty_like(self._flat)
        sc = self._acc_scratch
        again = torch.empty((self._max_batch, self.out_size), dtype=torch.float32, device=dout.device)       # the recomputed embeddings are not used
        for i, (lo, hi) in enumerate(passes[-1:] + passes[:-1]):
            if i:
                self._forward_pass(frames_u8, lo, hi, again[:hi - lo], boundary, reuse=True, windows=windows, color=color, blur=blur)
            _lib.check(L.pvr_trainer_backward_acc(self._handle, vp(self._flat), vp(dout[lo:hi]), dout.stride(0), vp(grads), 1 if i else 0, vp(sc), sc.numel(),
                                                  _lib.stream_ptr()))

    def _gather_pass(self, cache, rows, lo, hi):
        """rows[lo:hi] of the cache -> the first hi - lo rows of the staging tensor (made once: max_batch x boundary_floats)"""
        if self._staging is None:
            self._staging = torch.empty((self._max_batch, self._boundary_floats), dtype=torch.float32, device=cache.data.device)
        vp = lambda t: C.c_void_p(t.data_ptr())
        _lib.check(_lib.lib().pvr_op_gather_rows(vp(cache.data), cache.data.shape[0], self._boundary_floats, vp(rows[lo:hi]), hi - lo, vp(self._staging),
                                                 _lib.stream_ptr()))
        return self._staging

    def _forward_raw_cached(self, cache, rows):
        """_forward_raw on cache rows: per pass one gather into the staging tensor, then the pass from the first trained op on"""
        self.check_prefix_cache(cache)
        n = int(rows.numel())
        assert n >= 1 and rows.dim() == 1 and rows.dtype == torch.int64 and rows.is_contiguous()
        if n > self._max_batch and not self._freeze_bn:
            raise ValueError('training forward of %d frames: the workspace was made for max_batch = %d (BatchNorm takes the whole batch together, '
                             'it cannot be chunked)' % (n, self._max_batch))
        out = torch.empty((n, self.out_size), dtype=torch.float32, device=rows.device)
        for lo, hi in self._passes(n):            # (the staging tensor keeps the last pass's rows: its activations stay held for the backward)
            self._forward_pass(None, 0, hi - lo, out[lo:hi], self._gather_pass(cache, rows, lo, hi), reuse=True)
        return out

    def _backward_raw_cached(self, cache, rows, dout, grads):
        """_backward_raw on cache rows: the last pass first - the staging tensor still holds its rows - then every other pass in frame order, each
        gathered again, recomputed from the first trained op and added by pvr_trainer_backward_acc"""
        self.check_prefix_cache(cache)
        L = _lib.lib()
        vp = lambda t: C.c_void_p(t.data_ptr())
        passes = self._passes(int(rows.numel()))
        assert dout.shape[0] == rows.numel() and dout.stride(1) == 1
        if len(passes) == 1:
            _lib.check(L.pvr_trainer_backward(self._handle, vp(self._flat), vp(dout), dout.stride(0), vp(grads), _lib.stream_ptr()))
            return
        if self._acc_scratch is None:
            self._acc_scratch = torch.empty_like(self._flat)
        sc = self._acc_scratch
        again = torch.empty((self._max_batch, self.out_size), dtype=torch.float32, device=dout.device)       # the recomputed embeddings are not used
        for i, (lo, hi) in enumerate(passes[-1:] + passes[:-1]):
            if i:
                self._forward_pass(None, 0, hi - lo, again[:hi - lo], self._gather_pass(cache, rows, lo, hi), reuse=True)
            _lib.check(L.pvr_trainer_backward_acc(self._handle, vp(self._flat), vp(dout[lo:hi]), dout.stride(0), vp(grads), 1 if i else 0, vp(sc), sc.numel(),
                                                  _lib.stream_ptr()))

    def forward(self, frames_u8):
        if self.training:
            self.close()
            return _EncoderFunction.apply(self, frames_u8.contiguous(), *self._trained_plist)
        with torch.no_grad():
            return self._eval_model()(frames_u8)


TRAIN_FROM = ('layer1', 'layer2', 'layer3', 'layer4')


def resized_size(h, w, size):
    """(height, width) of an (h, w) frame after torchvision's resize(int size): the smaller edge becomes size, the other int(size * long / short)"""
    short, long_ = (w, h) if w <= h else (h, w)
    if short == size:
        return h, w
    new_long = int(size * long_ / short)
    return (new_long, size) if w <= h else (size, new_long)


def crop_windows(seed, call, n, max_top, max_left, first_frame=0):
    """the (n, 2) int32 windows (top, left) random_crop draws for frames first_frame .. first_frame + n of training forward number `call` under crop_seed
    `seed` (pvr_host_crop_windows: host arithmetic, no GPU needed; bit for bit what the device draws).  max_top, max_left: HipTrainableResNet.crop_range"""
    out = np.zeros((int(n), 2), np.int32)
    if n > 0:
        _lib.lib().pvr_host_crop_windows(int(seed), int(call), int(first_frame), int(n), int(max_top), int(max_left), out.ctypes.data_as(C.c_void_p))
    return out


def check_random_crop(random_crop, prefix_cache=False, what='prefix_cache'):
    """random_crop moves a frame's window from step to step: a ValueError together with the prefix cache (`what` names the keyword or the method)"""
    if random_crop and prefix_cache:
        raise ValueError('random_crop with %s: the cache holds the frozen prefix\'s output for ONE window per frame (the deterministic centre crop), and a '
                         'random crop moves the window in every step; prefix_once, which keeps the prefix\'s output for the frames and windows of one '
                         'step, is the compatible mode' % what)


def color_strengths(color_jitter):
    """the color_jitter keyword -> the (brightness, contrast, saturation) strengths as fp32 values, or None when the mode is off (None, 0 or all zeros); a
    scalar means all three.  A ValueError names a negative or non-finite strength, and a value that is neither a number nor three of them"""
    if color_jitter is None or color_jitter is False:
        return None
    try:
        v = tuple(float(x) for x in color_jitter) if hasattr(color_jitter, '__len__') else (float(color_jitter),) * 3
    except (TypeError, ValueError):
        v = ()
    if len(v) != 3:
        raise ValueError('color_jitter=%r: one strength for all of brightness, contrast and saturation, or the three of them (hue is not offered)'
                         % (color_jitter,))
    if not all(np.isfinite(x) and 0 <= x <= 3e38 for x in v):
        raise ValueError('color_jitter=%r: a strength is a finite number, 0 or above (a factor is drawn from [max(0, 1 - strength), 1 + strength]; 0 '
                         'leaves that factor at 1, and all zeros switch the mode off)' % (color_jitter,))
    v = tuple(float(np.float32(x)) for x in v)
    return v if any(v) else None


def color_params(seed, call, n, strengths, first_frame=0):
    """the n parameter rows color_jitter draws for frames first_frame .. first_frame + n of training forward number `call` under color_seed `seed`: a
    structured array with the fields b, c, s (float32 factors) and order (int32, 0 .. 5: the permutation of (brightness, contrast, saturation) in
    lexicographic order), 16 bytes per row as the device holds them.  pvr_host_color_params: host arithmetic, no GPU needed; bit for bit what the device
    draws.  strengths: a scalar or (b, c, s)"""
    v = color_strengths(strengths) or (0.0, 0.0, 0.0)
    out = np.zeros(int(n), COLOR_DTYPE)
    if n > 0:
        _lib.lib().pvr_host_color_params(int(seed), int(call), int(first_frame), int(n), v[0], v[1], v[2], out.ctypes.data_as(C.c_void_p))
    return out


COLOR_DTYPE = np.dtype([('b', np.float32), ('c', np.float32), ('s', np.float32), ('order', np.int32)])


def check_color_jitter(strengths, prefix_cache=False, what='prefix_cache'):
    """color_jitter changes a frame's image from step to step: a ValueError together with the prefix cache (`what` names the keyword or the method).
    strengths: what color_strengths returned"""
    if strengths is not None and prefix_cache:
        raise ValueError('color_jitter with %s: the cache holds the frozen prefix\'s output for ONE image per frame (the un-jittered centre crop), and the '
                         'jitter changes the image in every step; prefix_once, which keeps the prefix\'s output for the frames and images of one step, '
                         'is the compatible mode' % what)


def blur_spec(gaussian_blur):
    """the gaussian_blur keyword -> (p, sigma lo, sigma hi) as fp32 values, or None when the mode is off (None, False or p = 0).  A ValueError names a
    probability outside [0, 1] or not finite, a sigma range that is not finite or not 0 < lo <= hi, and a value that is not three numbers"""
    if gaussian_blur is None or gaussian_blur is False:
        return None
    try:
        v = tuple(float(x) for x in gaussian_blur)
    except (TypeError, ValueError):
        v = ()
    if len(v) != 3:
        raise ValueError('gaussian_blur=%r: three numbers (p, lo, hi) - the probability that a frame is blurred and the range its sigma is drawn from '
                         '(MoCo v2: (0.5, 0.1, 2.0); the kernel size is fixed at 23)' % (gaussian_blur,))
    if not (np.isfinite(v[0]) and 0 <= v[0] <= 1):
        raise ValueError('gaussian_blur=%r: the probability p = %r is a finite number in [0, 1] (0 switches the mode off)' % (gaussian_blur, v[0]))
    if not (np.isfinite(v[1]) and np.isfinite(v[2]) and 0 < v[1] <= v[2] <= 3e38):
        raise ValueError('gaussian_blur=%r: the sigma range (%r, %r) is finite with 0 < lo <= hi (the kernel clamps a sigma above 16)'
                         % (gaussian_blur, v[1], v[2]))
    v = tuple(float(np.float32(x)) for x in v)
    if not v[1] > 0:
        raise ValueError('gaussian_blur=%r: the sigma range\'s lo is 0 in fp32 (finite with 0 < lo <= hi)' % (gaussian_blur,))
    return v if v[0] > 0 else None


def gray_prob(random_grayscale):
    """the random_grayscale keyword -> the probability as an fp32 value, or None when the mode is off (None, False or 0).  A ValueError names a
    probability outside [0, 1] or not finite, and a value that is not a number"""
    if random_grayscale is None or random_grayscale is False:
        return None
    try:
        p = float(random_grayscale)
    except (TypeError, ValueError):
        raise ValueError('random_grayscale=%r: one number, the probability that a frame is replaced by its gray values (MoCo v2: 0.2)'
                         % (random_grayscale,))
    if not (np.isfinite(p) and 0 <= p <= 1):
        raise ValueError('random_grayscale=%r: a probability is a finite number in [0, 1] (0 switches the mode off)' % (random_grayscale,))
    p = float(np.float32(p))
    return p if p > 0 else None


BLUR_DTYPE = np.dtype([('sigma', np.float32), ('gray', np.int32)])


def blur_params(seed, call, n, gaussian_blur=None, random_grayscale=None, first_frame=0):
    """the n parameter rows gaussian_blur and random_grayscale draw for frames first_frame .. first_frame + n of training forward number `call` under
    blur_seed `seed`: a structured array with the fields sigma (float32, 0: not blurred) and gray (int32, 0 or 1), 8 bytes per row as the device holds
    them.  pvr_host_blur_params: host arithmetic, no GPU needed; bit for bit what the device draws.  gaussian_blur: (p, lo, hi) or None;
    random_grayscale: p or None"""
    b, g = blur_spec(gaussian_blur) or (0.0, 1.0, 1.0), gray_prob(random_grayscale) or 0.0
    out = np.zeros(int(n), BLUR_DTYPE)
    if n > 0:
        _lib.lib().pvr_host_blur_params(int(seed), int(call), int(first_frame), int(n), b[0], b[1], b[2], g, out.ctypes.data_as(C.c_void_p))
    return out


def check_gaussian_blur(blur, gray, prefix_cache=False, what='prefix_cache'):
    """gaussian_blur and random_grayscale change a frame's image from step to step: a ValueError together with the prefix cache (`what` names the
    keyword or the method).  blur, gray: what blur_spec and gray_prob returned"""
    for name, on in (('gaussian_blur', blur is not None), ('random_grayscale', gray is not None)):
        if on and prefix_cache:
            raise ValueError('%s with %s: the cache holds the frozen prefix\'s output for ONE image per frame (the plain centre crop), and the mode '
                             'changes the image in every step; prefix_once, which keeps the prefix\'s output for the frames and images of one step, '
                             'is the compatible mode' % (name, what))


def crop_scale(random_resized_crop):
    """the random_resized_crop keyword -> the (lo, hi) scale range as fp32 values, or None when the mode is off (None or False); a scalar s means (s, 1.0).
    A ValueError names a scale that is not finite or not 0 < lo <= hi <= 1, and a value that is neither a number nor two of them"""
    if random_resized_crop is None or random_resized_crop is False:
        return None
    try:
        v = tuple(float(x) for x in random_resized_crop) if hasattr(random_resized_crop, '__len__') else (float(random_resized_crop), 1.0)
    except (TypeError, ValueError):
        v = ()
    if len(v) != 2:
        raise ValueError('random_resized_crop=%r: the scale range (lo, hi) of the rectangle\'s share of the frame\'s area, or one number for (lo, 1.0) '
                         '(the ratio range is fixed at (3/4, 4/3))' % (random_resized_crop,))
    v = tuple(float(np.float32(x)) if np.isfinite(x) else x for x in v)
    if not (np.isfinite(v[0]) and np.isfinite(v[1]) and 0 < v[0] <= v[1] <= 1):
        raise ValueError('random_resized_crop=%r: a scale range is finite with 0 < lo <= hi <= 1 (the rectangle\'s area is uniform in [lo, hi] of the '
                         'frame\'s; MoCo\'s is (0.2, 1.0), and None switches the mode off)' % (random_resized_crop,))
    return v


def crop_rects(seed, call, n, h, w, scale, first_frame=0):
    """the (n, 4) int32 rectangles (top, left, height, width) random_resized_crop draws in (h, w) frames first_frame .. first_frame + n of training
    forward number `call` under crop_seed `seed` (pvr_host_crop_rects: host arithmetic, no GPU needed; bit for bit what the device draws).  scale: a
    scalar lo, for (lo, 1.0), or (lo, hi)"""
    v = crop_scale(scale)
    if v is None:
        raise ValueError('crop_rects: scale=%r (a scale range (lo, hi), or one number for (lo, 1.0))' % (scale,))
    if int(h) < 1 or int(w) < 1:
        raise ValueError('crop_rects: a %dx%d frame (both sizes are 1 or above)' % (h, w))
    out = np.zeros((int(n), 4), np.int32)
    if n > 0:
        _lib.lib().pvr_host_crop_rects(int(seed), int(call), int(first_frame), int(n), int(h), int(w), v[0], v[1], out.ctypes.data_as(C.c_void_p))
    return out


def check_random_resized_crop(scale, prefix_cache=False, what='prefix_cache', random_crop=False):
    """random_resized_crop changes a frame's image from step to step: a ValueError together with the prefix cache (`what` names the keyword or the
    method), and together with random_crop, which chooses the window too.  scale: what crop_scale returned"""
    if scale is not None and random_crop:
        raise ValueError('random_resized_crop with random_crop: both choose the frame\'s window - random_crop moves a 224 x 224 window in the frame after '
                         'Resize(256), random_resized_crop resizes a random rectangle of the original frame to 224 x 224; switch one of them off')
    if scale is not None and prefix_cache:
        raise ValueError('random_resized_crop with %s: the cache holds the frozen prefix\'s output for ONE window per frame (the deterministic centre crop), '
                         'and the rectangle changes in every step; prefix_once, which keeps the prefix\'s output for the frames and rectangles of one step, '
                         'is the compatible mode' % what)


def check_prefix_once(prefix_once, train_from):
    """prefix_once keeps the frozen prefix's boundary tensor across the passes of a step: a ValueError where nothing is frozen"""
    if prefix_once and train_from is None:
        raise ValueError('prefix_once needs train_from: with everything training there is no frozen prefix to keep (its one output is what the mode '
                         'caches across the passes of a step)')


def check_prefix_cache(prefix_cache, train_from):
    """prefix_cache computes the frozen prefix's boundary tensor once per dataset frame: a ValueError where nothing is frozen"""
    if prefix_cache and train_from is None:
        raise ValueError('prefix_cache needs train_from: with everything training there is no frozen prefix whose output could be cached for the '
                         'dataset\'s frames')


def train_stage(train_from):
    """pvr_trainer_set_train_from's stage of a train_from value: 0 for None, 1 .. 4 for 'layer1' .. 'layer4'; anything else is a ValueError"""
    if train_from is None:
        return 0
    if train_from not in TRAIN_FROM:
        raise ValueError("train_from %r: the choices are None (everything trains) or one of %s (that stage and the ones above it train)"
                         % (train_from, ', '.join(repr(x) for x in TRAIN_FROM)))
    return TRAIN_FROM.index(train_from) + 1


def require_trainable(embedding_name):
    """raise NotImplementedError unless `embedding_name` is one EmbeddingNet(..., train=True) is built for; returns its variant"""
    if embedding_name not in _SINGLE or _SINGLE[embedding_name][1] not in _TRAINABLE:
        raise NotImplementedError("training the embedding '%s' is not built: %s (the compressed *_l3 / *_l4 variants, Uber models, CLIP, MAE and "
                                  "'random' run frozen)" % (embedding_name, _TRAINABLE_MSG))
    return _SINGLE[embedding_name][1]


def _sizing_handle(embedding_name, max_batch):
    """a trainer handle made for a question of sizes (host arithmetic, no GPU needed); None when the trainer refuses that max_batch"""
    variant = require_trainable(embedding_name)
    L = _lib.lib()
    tr = transforms_for('')
    desc = _lib.EncoderDesc(arch=_ARCH[variant], dtype=_lib.PVR_F32, max_batch=int(max_batch), chunk=0, resize=tr.resize, crop=tr.crop)
    desc.mean[:] = tr.mean
    desc.std_[:] = tr.std
    h = C.c_void_p()
    if L.pvr_trainer_create(C.byref(desc), C.byref(h)) != 0:
        if 'largest max_batch' in _lib.last_error():
            return None
        _lib.check(1)
    return h


def trainer_boundary_bytes(embedding_name, train_from):
    """bytes per frame of the boundary tensor prefix_once keeps for a step's frames (pvr_trainer_boundary_floats on a handle made for the question:
    host arithmetic, no GPU needed); 0 when everything trains"""
    stage = train_stage(train_from)
    h = _sizing_handle(embedding_name, 1)
    L = _lib.lib()
    try:
        if stage:
            _lib.check(L.pvr_trainer_set_train_from(h, stage))
        return 4 * int(L.pvr_trainer_boundary_floats(h))
    finally:
        L.pvr_trainer_destroy(h)


def trainer_prefix_cache_bytes(embedding_name, train_from, n_frames):
    """bytes of the PrefixCache of n_frames dataset frames: n_frames x trainer_boundary_bytes (host arithmetic, no GPU needed).  The staging tensor of a
    cached pass (max_batch x trainer_boundary_bytes) lives next to it"""
    check_prefix_cache(True, train_from)
    return int(n_frames) * trainer_boundary_bytes(embedding_name, train_from)


def trainer_workspace_bytes(embedding_name, max_batch, wgrad_split16=False, conv_split16=False, train_from=None, prefix_once=False):
    """bytes of device memory the training workspace of `embedding_name` takes for max_batch frames (pvr_trainer_workspace_bytes on a handle made
    for the question: host arithmetic, no GPU needed), with fp32 or split-f16 weight gradients and convolutions, training everything or from train_from's stage up; None when the trainer refuses that max_batch (a
    tensor of the workspace would pass 2 GiB).  prefix_once: the workspace of that mode (with conv_split16 it holds no pre-BN tensor of the prefix); the
    boundary cache is the caller's and is counted by trainer_boundary_bytes"""
    stage = train_stage(train_from)
    check_prefix_once(prefix_once, train_from)
    L = _lib.lib()
    h = _sizing_handle(embedding_name, max_batch)
    if h is None:
        return None
    try:
        if prefix_once:
            _lib.check(L.pvr_trainer_set_prefix_fused(h, 1))
        if wgrad_split16:
            _lib.check(L.pvr_trainer_set_wgrad_split16(h, 1))
        if conv_split16:
            _lib.check(L.pvr_trainer_set_conv_split16(h, 1))
        if stage:
            _lib.check(L.pvr_trainer_set_train_from(h, stage))
        return int(L.pvr_trainer_workspace_bytes(h))
    finally:
        L.pvr_trainer_destroy(h)


def _get_trainable(embedding_name, pretrained, compute_dtype=None, max_batch=None, chunk=None, host=False, freeze_bn=False, wgrad_split16=False,
                   conv_split16=False, train_from=None, prefix_once=False, prefix_cache=False, random_crop=False, crop_seed=0, color_jitter=None,
                   color_seed=0, random_resized_crop=None, gaussian_blur=None, random_grayscale=None, blur_seed=0):
    """_get_embedding(..., train=True): the module for the scope the trainer is built for; everything else keeps raising NotImplementedError"""
    if embedding_name not in _SINGLE and embedding_name not in _UBER and embedding_name not in _CLIP and embedding_name not in _NOT_BUILT \
            and embedding_name not in ('random', 'mae_base', 'mae_large', 'mae_huge'):
        raise NotImplementedError("Requested model not available.")                 # embeddings.py:321
    require_trainable(embedding_name)
    train_stage(train_from)                       # (ValueError names the choices)
    check_prefix_once(prefix_once, train_from)
    check_prefix_cache(prefix_cache, train_from)
    check_random_crop(random_crop, prefix_cache)
    strengths = color_strengths(color_jitter)
    check_color_jitter(strengths, prefix_cache)
    rrc_scale = crop_scale(random_resized_crop)
    check_random_resized_crop(rrc_scale, prefix_cache, random_crop=random_crop)
    blur, gray = blur_spec(gaussian_blur), gray_prob(random_grayscale)
    check_gaussian_blur(blur, gray, prefix_cache)
    if host:
        raise NotImplementedError("training the embedding on the host backend (disable_cuda) is not built: %s" % _TRAINABLE_MSG)
    if compute_dtype is not None and _dtype_from_env(compute_dtype) != _lib.PVR_F32:
        raise ValueError("train=True computes in fp32 (compute_dtype None or 'f32'), got %r" % (compute_dtype,))
    sd, variant = _load_named_state_dict(embedding_name, pretrained)
    return HipTrainableResNet(sd, variant, max_batch=max_batch, freeze_bn=freeze_bn, wgrad_split16=wgrad_split16, conv_split16=conv_split16,
                              **({'train_from': train_from} if train_from is not None else {}), **({'prefix_once': True} if prefix_once else {}),
                              **({'prefix_cache': True} if prefix_cache else {}),
                              **({'random_crop': True, 'crop_seed': crop_seed} if random_crop else {}),
                              **({'color_jitter': strengths, 'color_seed': color_seed} if strengths else {}),
                              **({'random_resized_crop': rrc_scale, 'crop_seed': crop_seed} if rrc_scale else {}),
                              **({'gaussian_blur': blur} if blur else {}), **({'blur_seed': blur_seed} if blur or gray else {}),
                              **({'random_grayscale': gray} if gray else {}))


class UberModel(nn.Module):
    """reference src/embeddings.py:44-57.  `models` stays a plain list as in the reference (so, as there,
    its weights are not part of state_dict()); each member writes its columns of one output buffer."""

    def __init__(self, models):
        super().__init__()
        self.models = models
        assert all(models[0].training == m.training for m in models)
        self.training = models[0].training
        self.out_size = sum(m.out_size for m in models)

    def close(self):
        for m in self.models:
            m.close()

    def to(self, device):
        return self

    @property
    def lanes(self):
        return min(m.lanes for m in self.models)

    def set_crop(self, pos):
        for m in self.models:
            m.set_crop(pos)

    def set_low_latency(self, on=True):
        for m in self.models:
            m.set_low_latency(on)

    SMALL_BATCH = 16                  # at or below this many frames a member network leaves most of the GPU idle

    def forward_into(self, frames_u8, out, lane=0):
        """Members write their column blocks of `out`.  Small batches (online evaluation, EmbeddingWrapper: a handful of frames
        per call) run the members CONCURRENTLY on side streams forked from / joined to the caller's stream - each member is its
        own encoder with its own workspace; large batches run them one after the other (each already fills the GPU)."""
        cols, col = [], 0
        for m in self.models:
            cols.append((m, col))
            col += m.out_size
        if frames_u8.shape[0] > self.SMALL_BATCH or len(self.models) == 1:
            for m, c in cols:
                m.forward_into(frames_u8, out[:, c:c + m.out_size], lane=lane)
            return
        cur = torch.cuda.current_stream()
        if getattr(self, '_side', None) is None:
            self._side = [torch.cuda.Stream() for _ in self.models[1:]]
        for (m, c), st in zip(cols[1:], self._side):
            st.wait_stream(cur)
            with torch.cuda.stream(st):
                m.forward_into(frames_u8, out[:, c:c + m.out_size], lane=lane)
        m, c = cols[0]
        m.forward_into(frames_u8, out[:, c:c + m.out_size], lane=lane)
        for st in self._side:
            cur.wait_stream(st)

    def forward(self, frames_u8):
        out = torch.empty((frames_u8.shape[0], self.out_size), dtype=torch.float32, device=frames_u8.device)
        self.forward_into(frames_u8, out)
        return out


class FiveCrop(nn.Module):
    """Build-defined 5-crop extension (BASELINE config 5; the reference itself only has CenterCrop,
    embeddings.py:82): the wrapped model embeds the four corner windows and the centre window of the Resize(256) frame
    (torchvision FiveCrop order tl, tr, bl, br, centre) and the five embeddings are concatenated along the feature axis:
    (N, 5*O), the last O columns being exactly the reference's centre-crop embedding."""
    ORDER = (1, 2, 3, 4, 0)

    def __init__(self, model):
        super().__init__()
        self.model = [model]                                   # plain list: not a sub-module (as UberModel.models)
        self.training = model.training
        self.out_size = 5 * model.out_size

    def close(self):
        self.model[0].close()

    def to(self, device):
        return self

    @property
    def lanes(self):
        return self.model[0].lanes

    def forward_into(self, frames_u8, out, lane=0):
        m, o = self.model[0], self.model[0].out_size
        try:
            for k, pos in enumerate(self.ORDER):
                m.set_crop(pos)
                m.forward_into(frames_u8, out[:, k * o:(k + 1) * o], lane=lane)
        finally:
            m.set_crop(0)

    def forward(self, frames_u8):
        out = torch.empty((frames_u8.shape[0], self.out_size), dtype=torch.float32, device=frames_u8.device)
        self.forward_into(frames_u8, out)
        return out


class _Transforms(nn.Module):
    """Stand-in for the reference's nn.Sequential of torchvision transforms (embeddings.py:80-85, 309-314): it only records
    the parameters; the Resize / CenterCrop / ConvertImageDtype / Normalize arithmetic is fused into the HIP preprocess + stem
    (or patchify) kernels, which receive exactly these values through pvr_encoder_desc."""

    def __init__(self, resize=256, crop=224, mean=IMAGENET_MEAN, std=IMAGENET_STD, mode='bilinear', antialias=False):
        super().__init__()
        self.resize, self.crop, self.mean, self.std, self.mode, self.antialias = resize, crop, tuple(mean), tuple(std), mode, antialias

    def spec(self):
        """[op, args...] in application order - the form tests/golden/glue_registry.json records from the reference"""
        return [['Resize', self.resize, self.mode, self.antialias], ['CenterCrop', self.crop], ['ConvertImageDtype'],
                ['Normalize', [float(m) for m in self.mean], [float(x) for x in self.std]]]


def transforms_for(embedding_name):
    """The transforms the reference builds for a name: Resize(256) bilinear - bicubic if 'mae' is in the name (embeddings.py:81)
    - CenterCrop(224), /255, ImageNet Normalize (:80-85); the 'clip' names replace them by Resize(224, bicubic, antialias),
    CenterCrop(224), /255, CLIP Normalize (:309-314)."""
    if 'clip' in embedding_name:
        return _Transforms(224, 224, CLIP_MEAN, CLIP_STD, 'bicubic', True)
    return _Transforms(256, 224, IMAGENET_MEAN, IMAGENET_STD, 'bicubic' if 'mae' in embedding_name else 'bilinear', False)


def _get_embedding(embedding_name='random', in_channels=3, pretrained=True, train=False, **hip_kw):
    assert in_channels == 3, 'Current models accept 3-channel inputs only.'          # embeddings.py:87
    if embedding_name == 'true_state':
        return nn.Sequential(nn.Identity()), nn.Sequential(nn.Identity())
    if train:                                                                        # embeddings.py:323-326
        model = _get_trainable(embedding_name, pretrained, **hip_kw)
        model.train()
        for p in model.trained_parameters():      # (train_from: the frozen prefix keeps requires_grad = False)
            p.requires_grad = True
        return model, transforms_for(embedding_name)
    if embedding_name in _SINGLE:
        sd, variant = _load_named_state_dict(embedding_name, pretrained)
        model = HipResNet50(sd, variant, **hip_kw)
    elif embedding_name in _CLIP:
        variant, ckpt, patch = _CLIP[embedding_name]
        f = _find_checkpoint(ckpt) if pretrained else None
        if f is not None:                             # OpenAI's TorchScript archive: keep the visual tower only
            full = torch.jit.load(f, map_location='cpu').state_dict()
            sd = {k: v.float() for k, v in full.items() if k.startswith('visual.')}
        elif os.environ.get('PVR_SYNTHETIC_WEIGHTS', '0') == '1' or not pretrained:
            seed = zlib.crc32(embedding_name.encode()) & 0x7fffffff
            sd = synth.clip_rn50_state_dict(seed) if variant == 'clip_rn50' else synth.clip_vit_state_dict(seed, patch=patch)
        else:
            raise FileNotFoundError(ckpt)
        model = HipResNet50(sd, variant, **hip_kw)
    elif embedding_name == 'random':
        # embeddings.py:90-106: orthogonal(gain=relu) weights, zero bias, same constructor order -> same weights per torch seed
        init_ = lambda m: (nn.init.orthogonal_(m.weight.data, gain=nn.init.calculate_gain('relu')), nn.init.constant_(m.bias.data, 0), m)[2]
        layers, cin = [], in_channels
        for _ in range(5):
            layers += [init_(nn.Conv2d(cin, 32, kernel_size=(3, 3), stride=2, padding=1)), nn.ELU()]
            cin = 32
        model = HipResNet50(nn.Sequential(*layers).state_dict(), 'random5', **hip_kw)
    elif embedding_name in ('mae_base', 'mae_large', 'mae_huge'):   # embeddings.py:137-148; encoder keys only (strict=False there)
        ckpt, variant, patch, width, layers = {                                       # mae.py:275-296
            'mae_base': ('mae_pretrain_vit_base.pth', 'mae_b16', 16, 768, 12),
            'mae_large': ('mae_pretrain_vit_large.pth', 'mae_l16', 16, 1024, 24),
            'mae_huge': ('mae_pretrain_vit_huge.pth', 'mae_h14', 14, 1280, 32)}[embedding_name]
        f = _find_checkpoint(ckpt) if pretrained else None
        if f is not None:
            ck = torch.load(f, map_location='cpu')['model']
            sd = {k: v.float() for k, v in ck.items() if not k.startswith(('decoder', 'mask_token'))}
            sd.setdefault('pos_embed', torch.from_numpy(synth.sincos_2d_pos_embed(width, 224 // patch)[None]))     # fixed buffer
        elif os.environ.get('PVR_SYNTHETIC_WEIGHTS', '0') == '1' or not pretrained:
            sd = synth.mae_vit_state_dict(zlib.crc32(embedding_name.encode()) & 0x7fffffff, patch=patch, width=width, layers=layers)
        else:
            raise FileNotFoundError(ckpt)
        model = HipResNet50(sd, variant, **hip_kw)
    elif embedding_name in _UBER:
        model = UberModel([_get_embedding(n, in_channels, pretrained, train, **hip_kw)[0] for n in _UBER[embedding_name]])
    elif embedding_name in _NOT_BUILT:
        raise NotImplementedError("Requested model not available. ('%s' is registered by the reference but its "
                                  "family is not built in pvr_habitat_amd yet)" % embedding_name)
    else:
        raise NotImplementedError("Requested model not available.")                 # embeddings.py:321
    model.eval()
    for p in model.parameters():
        p.requires_grad = False
    return model, transforms_for(embedding_name)


class EmbeddingNet(nn.Module):
    """
    Input shape must be (N, H, W, 3), where N is the number of frames.
    The output shape will be (N, O), where O is the embedding size.   (reference embeddings.py:339-402)
    """

    def __init__(self, embedding_name, in_channels=3, pretrained=True, train=False, disable_cuda=False,
                 compute_dtype=None, max_batch=None, chunk=None, crops=1, freeze_bn=False, wgrad_split16=False, conv_split16=False, train_from=None,
                 prefix_once=False, prefix_cache=False, random_crop=False, crop_seed=0, color_jitter=None, color_seed=0, random_resized_crop=None,
                 gaussian_blur=None, random_grayscale=None, blur_seed=0):
        super(EmbeddingNet, self).__init__()
        self.embedding_name = embedding_name
        if self.embedding_name == 'true_state':
            return
        self.in_channels = in_channels
        # disable_cuda: the reference then runs on the CPU (embeddings.py:367-370); here that is the library's host backend
        # (csrc/host_encoder.hip: plain C++ loops behind the same pvr_encoder_* ABI, fp32) - the ResNet family only.
        # It is selected EXPLICITLY (the reference's own flag); a box whose GPU is missing or invisible still fails loudly (no silent fallback).
        self._host = bool(disable_cuda)
        if crops == 5 and train:
            raise NotImplementedError('train=True with crops=5: the 5-crop extension wraps the frozen encoder only')
        if freeze_bn and not train:
            raise ValueError('freeze_bn is a mode of the trainable encoder (train=True): a frozen encoder already runs on the running statistics')
        if wgrad_split16 and not train:
            raise ValueError('wgrad_split16 is a mode of the trainable encoder (train=True): a frozen encoder computes no weight gradient')
        if conv_split16 and not train:
            raise ValueError('conv_split16 is a mode of the trainable encoder (train=True): a frozen encoder has its own plans (compute_dtype \'f32s\' is '
                             'the split-f16 one)')
        if train_from is not None and not train:
            raise ValueError('train_from is a mode of the trainable encoder (train=True): a frozen encoder trains nothing')
        train_stage(train_from)                   # (ValueError names the choices)
        if prefix_once and not train:
            raise ValueError('prefix_once is a mode of the trainable encoder (train=True, with train_from): a frozen encoder has no training step and '
                             'no frozen prefix to keep across its passes')
        check_prefix_once(prefix_once, train_from)
        if prefix_cache and not train:
            raise ValueError('prefix_cache is a mode of the trainable encoder (train=True, with train_from): a frozen encoder has no training step and '
                             'no frozen prefix whose output could be cached')
        check_prefix_cache(prefix_cache, train_from)
        if random_crop and not train:
            raise ValueError('random_crop is a mode of the trainable encoder (train=True): a frozen encoder embeds the centre crop of every frame (crops=5 '
                             'adds the four corner windows)')
        check_random_crop(random_crop, prefix_cache)
        strengths = color_strengths(color_jitter)                # (a ValueError names a negative or non-finite strength)
        if strengths is not None and not train:
            raise ValueError('color_jitter is a mode of the trainable encoder (train=True): a frozen encoder embeds the un-jittered centre crop of every '
                             'frame')
        check_color_jitter(strengths, prefix_cache)
        rrc_scale = crop_scale(random_resized_crop)              # (a ValueError names a bad scale)
        if rrc_scale is not None and not train:
            raise ValueError('random_resized_crop is a mode of the trainable encoder (train=True): a frozen encoder embeds the centre crop of every frame '
                             '(crops=5 adds the four corner windows)')
        check_random_resized_crop(rrc_scale, prefix_cache, random_crop=random_crop)
        blur, gray = blur_spec(gaussian_blur), gray_prob(random_grayscale)      # (a ValueError names a bad probability or sigma range)
        for name, on in (('gaussian_blur', blur), ('random_grayscale', gray)):
            if on is not None and not train:
                raise ValueError('%s is a mode of the trainable encoder (train=True): a frozen encoder embeds the plain centre crop of every frame' % name)
        check_gaussian_blur(blur, gray, prefix_cache)
        # gaussian_blur, random_grayscale (train=True only): a training forward grays and blurs frames with the given probabilities; blur_seed keys the draw
        # random_resized_crop (train=True only): a training forward resizes a random rectangle of every frame to the crop; crop_seed keys the draw
        # color_jitter (train=True only): a training forward jitters brightness, contrast and saturation per frame; color_seed keys the draw
        # random_crop (train=True only): a training forward crops a random window per frame; crop_seed keys the draw (HipTrainableResNet.crop_call counts it)
        # prefix_cache (train=True with train_from only): the workspace mode of cached steps (build_prefix_cache / forward_cached of the encoder)
        # prefix_once (train=True with train_from only): the frozen prefix runs once per frame and step; its boundary tensor is kept across the passes
        # train_from (train=True only): partial fine-tuning - that stage and the ones above train, everything below is the frozen prefix
        # freeze_bn (train=True only): frozen BatchNorm, max_batch is then the chunk of a training forward (HipTrainableResNet)
        # wgrad_split16 (train=True only): the weight gradients as exact-split products on the f16 matrix pipe
        # conv_split16 (train=True only): the forward convolutions and the data gradients of layer1 .. layer4 as such products
        self.embedding, self.transforms = _get_embedding(embedding_name, in_channels, pretrained, train, compute_dtype=compute_dtype, max_batch=max_batch,
                                                         chunk=chunk, host=self._host, **({'freeze_bn': True} if freeze_bn else {}),
                                                         **({'wgrad_split16': True} if wgrad_split16 else {}),
                                                         **({'conv_split16': True} if conv_split16 else {}),
                                                         **({'train_from': train_from} if train_from is not None else {}),
                                                         **({'prefix_once': True} if prefix_once else {}),
                                                         **({'prefix_cache': True} if prefix_cache else {}),
                                                         **({'random_crop': True, 'crop_seed': crop_seed} if random_crop else {}),
                                                         **({'color_jitter': strengths, 'color_seed': color_seed} if strengths else {}),
                                                         **({'random_resized_crop': rrc_scale, 'crop_seed': crop_seed} if rrc_scale else {}),
                                                         **({'gaussian_blur': blur} if blur else {}), **({'blur_seed': blur_seed} if blur or gray else {}),
                                                         **({'random_grayscale': gray} if gray else {}))
        assert crops in (1, 5), 'crops: 1 (the reference CenterCrop) or 5 (corner + centre windows, FiveCrop order)'
        if crops == 5:
            self.embedding = FiveCrop(self.embedding)
        # the reference discovers these with a dummy CPU forward (embeddings.py:359-363)
        self.in_shape = torch.Size((in_channels, 224, 224))
        self.out_size = int(self.embedding.out_size)
        self.device = torch.device('cpu') if self._host else torch.device('cuda')
        self.training = self.embedding.training

    def _forward(self, observation_u8):
        return self.embedding(observation_u8)

    def set_bn_frozen(self, on=True):
        """frozen BatchNorm of the trainable encoder on / off (HipTrainableResNet.set_bn_frozen)"""
        if not isinstance(self.embedding, HipTrainableResNet):
            raise NotImplementedError('set_bn_frozen: only the trainable encoder (train=True) has a BatchNorm mode; %s' % _TRAINABLE_MSG)
        self.embedding.set_bn_frozen(on)

    def close(self):
        """free every library handle under this embedding now (HipResNet50.close); the module stays usable"""
        for m in self.modules():
            if m is not self and hasattr(m, 'close'):
                m.close()

    def embed_device(self, observation):
        """uint8 (N,H,W,3) -> fp32 (N, out_size) on self.device (cuda; host memory for a host-backend encoder); no host sync (for streaming callers)."""
        if not self._host:
            _lib.require_gpu()
        observation = observation.to(device=self.device, non_blocking=True).contiguous()
        if not self._host and not getattr(self, '_range_checked', False):
            self._range_checked = True
            self.validate_range(observation)
        return self._forward(observation)

    def validate_range(self, observation_dev, max_frames=8):
        """ONE-OFF, on the first frames this net embeds (PVR_RANGE_CHECK=0 skips it): every f16 or f32s ResNet member runs pvr_encoder_check_range on up to
        `max_frames` of them.  The reference is fp32 (src/embeddings.py:386-402); f16 storage has 5 exponent bits, and an activation that overflows inside the
        network can come out as a finite, wrong embedding (ReLU maps -inf and NaN to 0) - this names the convolution instead.  It validates THESE frames with
        THIS checkpoint, not every later batch; the per-batch finite check of the outputs stays."""
        if os.environ.get('PVR_RANGE_CHECK', '1') == '0':
            return
        members = []
        for m in [self.embedding] + [x for x in getattr(self.embedding, 'model', [])]:
            members += list(getattr(m, 'models', [m]))
        for m in members:
            if isinstance(m, HipResNet50) and m._dtype in (_lib.PVR_F16, _lib.PVR_F32S) and m.variant in ('conv5', 'conv4', 'conv3', 'r18', 'r34'):
                bad = m.check_range(observation_dev[:max_frames])
                if bad is not None and m._dtype == _lib.PVR_F32S:
                    raise FloatingPointError("activations of '%s' leave the f16 range of the split product's high parts on these frames (first output above "
                                             "65504: %s): use compute_dtype='f32' (full fp32 range) for this checkpoint" % (self.embedding_name, bad))
                if bad is not None:
                    raise FloatingPointError("activations of '%s' leave the f16 range on these frames (first non-finite output: %s): "
                                             "use compute_dtype='bf16' (8 exponent bits) or 'f32' for this checkpoint" % (self.embedding_name, bad))

    def forward(self, observation):
        if self.embedding_name == 'true_state':
            return observation.squeeze().cpu().numpy()
        # observation.shape -> (N, H, W, 3); transposes + transforms + model are one HIP plan
        # embeddings.py:396-398: a device tensor that keeps its graph.  Only the trainable module has a training mode: a frozen encoder on which
        # .train() was called (by a parent module, say) keeps returning checked numpy rows
        if isinstance(self.embedding, HipTrainableResNet) and self.embedding.training:
            out = self.embed_device(observation)
            return out.view(-1, self.out_size).squeeze()
        with torch.no_grad():
            out = self.embed_device(observation)
            return _checked(out.view(-1, self.out_size).squeeze().cpu().numpy(), self.embedding)


def _checked(host_out, model):
    """The embeddings are on the host anyway: a non-finite value means an activation left the 16-bit storage range (f16 has
    5 exponent bits; the reference computes in fp32).  Fail loudly instead of handing garbage to the BC stage."""
    if not np.isfinite(host_out).all():
        dt = getattr(model, '_dtype', None)
        if dt == _lib.PVR_F32S:
            raise FloatingPointError("non-finite embedding: activations overflowed the f16 high parts of the split product (f32s); "
                                     "use compute_dtype='f32' (full fp32 range) for this checkpoint")
        raise FloatingPointError('non-finite embedding: activations overflowed the encoder storage type (%s); '
                                 "use compute_dtype='bf16' (8 exponent bits) or 'f32' for this checkpoint"
                                 % {_lib.PVR_F16: 'f16', _lib.PVR_BF16: 'bf16', _lib.PVR_F32: 'f32', _lib.PVR_F32S: 'f32s'}.get(dt, 'mixed'))
    return host_out


_STREAM_CACHE = {}
_REGISTER_MIN_BYTES = 64 << 20      # stream_embed page-locks a pageable source in place only from this size up (see there)


def _streams(dev_index=None):
    """The four side streams this package uses (two compute lanes, H2D, D2H), created ONCE per device and process, together and in
    this order.  HIP maps streams onto a few hardware queues at creation; which queue a stream lands on changes what overlaps with
    what (scripts/stream_queue_ab.py, stream_embed from pinned memory in a fresh process: creation order lanes-then-copies 77.8 k
    frames/s, copies-then-lanes 56.1 k; bench.py: a leg on two freshly created streams ran at the one-lane rate, 69.8 k instead of
    79.8 k).  Every user of side streams in this package (stream_embed, bench.py's legs) takes them from here, so the process
    has one fixed, known-good set instead of whatever the creation history produced."""
    if dev_index is None:
        dev_index = torch.cuda.current_device()
    if dev_index not in _STREAM_CACHE:
        # a / b = compute lanes, h = H2D, d = D2H, x = a spare stream that is never used.  'xabhd' was the one order that measured the
        # full rate in every context tried (fresh process, after other streams, four and eight hardware queues; 'abhd' and 'hdab' each lose
        # 25 % in one of them): profiles/experiments/r02_stream_creation_order.txt
        order = os.environ.get('PVR_STREAM_ORDER', 'xabhd')
        made = {}
        with torch.cuda.device(dev_index):
            for ch in order:
                made[ch if ch != 'x' else 'x%d' % len(made)] = torch.cuda.Stream()
        _STREAM_CACHE[dev_index] = (made['h'], made['d'], [made['a'], made['b']], made)
    return _STREAM_CACHE[dev_index][:3]


def lane_streams(dev_index=None):
    """the two compute-lane streams (batch k+1 on lane 1 while batch k drains on lane 0)"""
    return list(_streams(dev_index)[2])


def _stage_rows(dst, x, lo, m, threads):
    """x[lo:lo+m] (uint8, host, possibly a channel-plane view of interleaved frames) -> the pinned tensor dst[:m], by the library's native
    threads (pvr_stage_copy; the call releases the GIL).  Layouts it does not know fall back to torch's copy."""
    src = x[lo:lo + m]
    row = int(np.prod(src.shape[1:]))
    st = src.stride()
    if src.is_contiguous():
        _lib.check(_lib.lib().pvr_stage_copy(C.c_void_p(dst.data_ptr()), C.c_void_p(src.data_ptr()), m, row, row, row, row, threads))
    elif (src.dim() == 4 and src.shape[3] == 3 and st[3] == 1 and st[2] >= 3 and st[1] == src.shape[2] * st[2] and
          (m == 1 or st[0] >= src.shape[1] * st[1])):
        # one 3-channel plane of (N, H, W, 3F) frames: runs of 3 bytes every 3F bytes
        _lib.check(_lib.lib().pvr_stage_copy(C.c_void_p(dst.data_ptr()), C.c_void_p(src.data_ptr()), m, row, st[0] if m > 1 else row, 3, st[2], threads))
    else:
        dst[:m].copy_(src)


def stream_embed(net, frames_u8, batch=256, out=None, depth=4, stage_threads=None, planes=1):
    """Embed a large uint8 (N,H,W,3) array - host-resident, or a CUDA tensor (then only the compute and D2H stages run) - with H2D copies, HIP compute and D2H copies overlapped: a ring of `depth`
    device input / output buffers, one copy stream each way and TWO compute streams (each on its own encoder workspace lane, so
    batch k+1 starts while batch k drains) chained by events.  The ring is deeper than the number of batches in flight on the
    compute side: with only one buffer per lane the upload of batch k+2 cannot start before batch k has been computed, and the lane
    then idles for the whole copy (measured: 60 k frames/s at 11.8 GB/s on a link that sustains 56 GB/s).  Pageable sources are
    staged through pinned buffers by the library's native threads (pvr_stage_copy, `stage_threads` of them, default PVR_STAGE_THREADS
    or 8: one memcpy thread moves ~3 GB/s) on a PRODUCER thread that runs up to `depth` batches ahead of the thread that enqueues the
    GPU work (round 3 staged synchronously between two enqueues: 36 k frames/s from pageable memory).  Same rows, same order, same
    values as calling `net` batch by batch; this is the "embeddings streamed to host" path of BASELINE config 5 and what
    save_embedded_obs uses for big scenes.  Returns np.float32 (N, planes * out_size) (no squeeze).

    planes = F > 1: frames_u8 is (N,H,W,3F) (the scene pickles hold current + goal frame interleaved, save_embedded_obs.py:148-150);
    a batch of whole rows is uploaded ONCE, each 3-channel plane is sliced on the device and embedded into its column block of the
    output row - what the reference builds with np.split / np.concatenate around its model call (:151-156)."""
    _lib.require_gpu()
    if stage_threads is None:
        stage_threads = int(os.environ.get('PVR_STAGE_THREADS', '8'))
    # a strided view (e.g. the channel slice obs[..., 3:6] of a (N,H,W,6) scene) is taken as it is: the staging threads gather it
    # into pinned memory batch by batch, overlapped with the GPU, instead of one np.ascontiguousarray pass over the scene up front
    x = frames_u8 if isinstance(frames_u8, torch.Tensor) else torch.from_numpy(frames_u8 if all(st >= 0 for st in frames_u8.strides)
                                                                               else np.ascontiguousarray(frames_u8))
    F_ = int(planes)
    assert x.dtype == torch.uint8 and x.dim() == 4 and x.shape[3] == 3 * F_
    n, osz = x.shape[0], net.out_size
    res = torch.empty((n, F_ * osz), dtype=torch.float32, pin_memory=True) if out is None else out
    assert tuple(res.shape) == (n, F_ * osz)
    dev = torch.device('cuda')
    if os.environ.get('PVR_STREAM_FRESH', '0') == '1':       # experiment: new streams per call
        h2d, d2h, comps = torch.cuda.Stream(), torch.cuda.Stream(), [torch.cuda.Stream(), torch.cuda.Stream()]
    else:
        h2d, d2h, comps = _streams(torch.cuda.current_device())
        comps = list(comps)
    for s_ in (h2d, d2h, *comps):
        s_.wait_stream(torch.cuda.current_stream())          # whatever the caller queued (e.g. a forward on the default stream) comes first
    model = net.embedding
    if hasattr(net, 'validate_range') and not getattr(net, '_range_checked', False) and not getattr(net, '_host', False) and n > 0:
        net._range_checked = True                           # the one-off f16 range validation on the first frames of the stream (EmbeddingNet.validate_range)
        net.validate_range(x[:8, :, :, :3].to(device=dev).contiguous())
    two_lanes = getattr(model, 'lanes', 1) >= 2 and os.environ.get('PVR_STREAM_LANES', '2') != '1'
    depth = max(2, min(int(depth), (n + batch - 1) // batch + 1))
    device_src = x.is_cuda                                  # frames already in HBM (PNG source decoded on the GPU): no upload at all
    pinned_src = device_src or (x.is_pinned() and (F_ > 1 or x.is_contiguous()))   # caller already holds page-locked frames: no staging copy
    registered = None
    if (not pinned_src and stage_threads != 0 and os.environ.get('PVR_STREAM_REGISTER', '0') == '1' and x.is_contiguous()
            and x.numel() >= _REGISTER_MIN_BYTES):
        # OPT-IN (PVR_STREAM_REGISTER=1): page-lock the caller's array IN PLACE for the duration of the call (hipHostRegister), so the
        # frames go straight from the caller's memory to the GPU by DMA - no staging copy.  Round 2 did this by default for any
        # pageable source, i.e. it locked and unlocked pages of the glibc heap that the package does not own, next to unrelated objects
        # (ADVICE round 2); now it needs the opt-in AND a buffer of >= 64 MiB, which glibc serves by a private mmap (above
        # M_MMAP_THRESHOLD_MAX), so the locked pages belong to this array alone.
        try:
            if int(torch.cuda.cudart().cudaHostRegister(x.data_ptr(), x.numel(), 0)) == 0:
                registered = x.data_ptr()
                pinned_src = True
        except Exception:
            registered = None
    shape = (batch,) + tuple(x.shape[1:])
    direct = pinned_src or stage_threads == 0              # stage_threads = 0: hand pageable memory to the driver's own staged copy
    stage_in = None if direct else [torch.empty(shape, dtype=torch.uint8, pin_memory=True) for _ in range(depth)]
    dev_in = None if device_src else [torch.empty(shape, dtype=torch.uint8, device=dev) for _ in range(depth)]
    dev_pl = [torch.empty(shape[:3] + (3,), dtype=torch.uint8, device=dev) for _ in range(2)] if F_ > 1 else None   # one plane, per lane
    dev_out = [torch.empty((batch, F_ * osz), dtype=torch.float32, device=dev) for _ in range(depth)]
    bad_flag = torch.zeros(1, dtype=torch.int32, device=dev)   # set on the device by any batch that holds an inf / NaN (pvr_op_nonfinite_flag); read once at the end
    for s_ in comps:
        s_.wait_stream(torch.cuda.current_stream())          # (the zero fill above)
    in_free = [torch.cuda.Event() for _ in range(depth)]    # compute finished reading dev_in[b]
    out_free = [torch.cuda.Event() for _ in range(depth)]   # D2H finished reading dev_out[b]
    for e in in_free + out_free:
        e.record()
    starts = list(range(0, n, batch))

    # producer thread: pageable -> pinned staging slot, up to `depth` batches ahead; a slot returns to it with the event that marks the end
    # of the H2D copy that read it
    import queue
    import threading
    free_q, ready_q = queue.Queue(), queue.Queue()
    stop = threading.Event()

    def producer():
        try:
            for i, lo in enumerate(starts):
                b, ev = free_q.get()
                if stop.is_set():
                    return
                if ev is not None:
                    ev.synchronize()                             # the upload that last read this slot has finished
                m = min(batch, n - lo)
                _stage_rows(stage_in[b], x, lo, m, max(1, stage_threads))
                ready_q.put((i, b))
        except BaseException as exc:                             # noqa: BLE001 - handed to the consuming thread
            ready_q.put(exc)

    worker = None
    if not direct:
        for b in range(depth):
            free_q.put((b, None))
        worker = threading.Thread(target=producer, name='pvr-stage', daemon=True)
        worker.start()

    try:
        for i, lo in enumerate(starts):
            m = min(batch, n - lo)
            if direct:
                b = i % depth
                src = x[lo:lo + m]
            else:
                got = ready_q.get()
                if isinstance(got, BaseException):
                    raise got
                assert got[0] == i
                b = got[1]
                src = stage_in[b][:m]
            if not device_src:
                with torch.cuda.stream(h2d):
                    h2d.wait_event(in_free[b])
                    dev_in[b][:m].copy_(src, non_blocking=True)
                    ready = torch.cuda.Event(); ready.record(h2d)
                if not direct:
                    free_q.put((b, ready))                        # the staging slot is reusable once this upload has read it
            lane = (i & 1) if two_lanes else 0
            comp = comps[lane]
            with torch.cuda.stream(comp):
                if not device_src:
                    comp.wait_event(ready)
                comp.wait_event(out_free[b])
                rows = src if device_src else dev_in[b][:m]
                if F_ == 1:
                    model.forward_into(rows, dev_out[b][:m], lane=lane)
                else:
                    for f in range(F_):
                        dev_pl[lane][:m].copy_(rows[..., 3 * f:3 * f + 3])       # plane f, contiguous (same stream: ordered before its forward)
                        model.forward_into(dev_pl[lane][:m], dev_out[b][:m, f * osz:(f + 1) * osz], lane=lane)
                in_free[b].record(comp)
                # finite check of this batch on the device, behind its forwards on the same stream (a host pass over the whole result at the
                # end cost 19 % of the 5-crop uber leg's wall clock: 31 310 floats per frame)
                _lib.check(_lib.lib().pvr_op_nonfinite_flag(C.c_void_p(dev_out[b].data_ptr()), m, F_ * osz, dev_out[b].stride(0),
                                                            C.c_void_p(bad_flag.data_ptr()), C.c_void_p(comp.cuda_stream)))
                done = torch.cuda.Event(); done.record(comp)
            with torch.cuda.stream(d2h):
                d2h.wait_event(done)
                res[lo:lo + m].copy_(dev_out[b][:m], non_blocking=True)
                out_free[b].record(d2h)
        torch.cuda.synchronize()
    finally:
        stop.set()
        if worker is not None:
            free_q.put((0, None))                                 # wake a producer that waits for a slot
            worker.join()
        if registered is not None:
            torch.cuda.synchronize()
            rc = int(torch.cuda.cudart().cudaHostUnregister(registered))
            if rc != 0:
                import warnings
                warnings.warn('stream_embed: hipHostUnregister(%#x) returned %d - the source array stays page-locked' % (registered, rc))
    if int(bad_flag.item()) != 0:
        _checked(res.numpy(), model)                          # raises FloatingPointError naming the storage type (and locates nothing else)
        raise FloatingPointError('non-finite embedding in the streamed result')
    return res.numpy() if out is None else res


try:                                          # the reference subclasses gym.ObservationWrapper (embeddings.py:409); gym is optional here
    import gym as _gym
    from gym.spaces.box import Box as _Box
    _WrapperBase = _gym.ObservationWrapper
except Exception:                             # no gym in this image: same attributes, no simulator dependency
    _gym = None

    class _Box(object):
        """the two attributes of gym.spaces.Box the BC scripts read (`.shape`, main_bc_2.py:76; `.low/.high`)"""

        def __init__(self, low, high, shape):
            self.low, self.high, self.shape, self.dtype = low, high, tuple(shape), np.float32

    class _WrapperBase(object):
        """gym.Wrapper's surface as far as the reference uses it: `.env`, attribute forwarding, reset/step through
        `observation()` (gym.ObservationWrapper.reset / step)."""

        def __init__(self, env):
            self.env = env
            self.observation_space = getattr(env, 'observation_space', None)
            self.action_space = getattr(env, 'action_space', None)

        def __getattr__(self, name):
            if name.startswith('_') or name == 'env':
                raise AttributeError(name)
            return getattr(self.env, name)

        def reset(self, **kwargs):
            return self.observation(self.env.reset(**kwargs))

        def step(self, action):
            observation, reward, done, info = self.env.step(action)
            return self.observation(observation), reward, done, info


class EmbeddingWrapper(_WrapperBase):
    """reference src/embeddings.py:409-444: places the embedding over the observation.  The original observation shape must be
    (H, W, n * 3); each of the n frames passes through the embedding separately and the outputs are stacked:
    `observation((H,W,3n)) -> (n*O,)`, `observation_space = Box(-inf, inf, shape=(O*n,))`.  Subclasses gym.ObservationWrapper
    when gym is importable, otherwise a base with the same surface.  The n frames go to the GPU as ONE batch."""

    def __init__(self, env, embedding):
        _WrapperBase.__init__(self, env)
        in_channels = env.observation_space.shape[2]
        assert in_channels % 3 == 0, \
            """ Only RGB images are supported.
                    Be sure that observation shape is (H, W, n * 3),
                    where n is the number of frames per observation. """
        self.in_channels = 3
        self.n_frames = in_channels // 3
        self.embedding = embedding
        self.observation_space = _Box(low=-np.inf, high=np.inf, shape=(self.embedding.out_size * self.n_frames,))
        # one environment step = one forward of n_frames (2) frames: ask the HIP encoder for its low-latency plan for such calls
        # (larger batches through the same EmbeddingNet are unaffected)
        model = getattr(self.embedding, 'embedding', None)
        if hasattr(model, 'set_low_latency'):
            model.set_low_latency(True)

    def observation(self, observation):
        # (H, W, n_frames * 3) -> (n_frames, H, W, 3); if n_frames > 1, each passes through the embedding separately
        observation = np.stack(np.split(observation, self.n_frames, axis=-1))
        return self.embedding(torch.from_numpy(observation)).flatten()
