"""The Stage-II SPADE refiner: drop-ins for ``SPADELayer``, ``SPADEBlock``, the generators built from them, of the
reference's ``nerf/_init_spade.py`` (:114-160, :235-282) with the reference's ``state_dict`` layout (including the duplicated
``conv1`` / ``conv1_sn`` entries: the reference registers each spectral-normalised convolution under two names), so its checkpoints load.

What runs where (DESIGN.md sections 8, 9): the 3x3 convolutions are library work -- ``torch.nn.functional.conv2d`` is MIOpen on ROCm --
forward and backward, in fp32 and under bf16 autocast.  That was judged for the fp32 forward and has since been measured for the bf16
backward: of the 231 ms autocast training step the GPU works 29 ms, the library's bf16 convolution backward is faster than its fp32
one, and MFMA kernels written for it were 2 ms per step slower than the library's (the step's 200 ms are host time of spectral norm's
bf16 matrix-vector products: section 9; ``fuse_spectral_norm_`` is the opt-in that takes them, and torch's ~350 small launches per step,
onto one fused op with sigma in fp32).  The normalise / modulate / activate chain between them, which the reference runs as
six elementwise passes, is ONE fused HIP kernel behind a statistics pass (``ops.spade_modulate``).  It is differentiable -- a fused
two-launch backward in place of six autograd nodes per SPADE layer -- so the generators train: ``refine_step`` is the step of the
reference's train_get_texture_photo.py / train_get_texture_photo_audio.py (clamp, MSE, Adam; the discriminator and the VGG loss that
_init_spade.py also defines are never called by those loops and are not built).

Inference: ``freeze_identity`` computes once what depends on the identity photo alone -- the IdEncoder, the gamma /
beta convolutions of the SPADE layers it feeds, the eval-mode spectral-normalised weights -- and ``refine_frames`` is the loop of
eval_get_texture_photo.py / eval_get_texture_photo_audio.py over the resulting ``FrozenRefiner``, whose modulation is
``ops.spade_modulate_frozen`` (one gamma / beta map for a batch of frames, the nearest 2x upsamples read in place).
"""
import contextlib
import os

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.nn.utils import spectral_norm
from torch.nn.utils.spectral_norm import SpectralNorm

from . import ops


def _conv3(cin, cout, stride=1):
    return nn.Conv2d(cin, cout, 3, stride, 1)


class TiledCodeMap:
    """The modulation map Generator_audio builds from the audio code (_init_spade.py:366-370): the 64-vector repeated to a (1, channels, height,
    64 * tiles) tensor -- every channel and every row the same, the code tiled along the width; the reference materialises it (268 MB for
    its 256 x 64 x 4096) and lets every SPADELayer resize it by nearest neighbour.  Here it stays the 64 numbers: ``nearest(size)`` returns
    what ``F.interpolate(materialised, size, mode="nearest")`` returns, computed from ATen's own index rule."""

    def __init__(self, code, channels, height, tiles):
        self.code, self.channels, self.height, self.tiles = code.reshape(-1), int(channels), int(height), int(tiles)

    @staticmethod
    def _nearest_index(out_size, in_size):
        """ATen upsample_nearest (non-exact mode): min(floor(dst * float32(in / out)), in - 1), evaluated in float32 as ATen does."""
        import numpy as np
        scale = np.float32(in_size) / np.float32(out_size)
        idx = np.floor(np.arange(out_size, dtype=np.float32) * scale).astype(np.int64)
        return np.minimum(idx, in_size - 1)

    def nearest(self, size):
        h, w = int(size[0]), int(size[1])
        cols = torch.from_numpy(self._nearest_index(w, self.code.numel() * self.tiles) % self.code.numel()).to(self.code.device)
        return self.code[cols].reshape(1, 1, 1, w).expand(1, self.channels, h, w).contiguous()

    def materialise(self):
        """The reference's tensor (tests compare ``nearest`` against interpolating this)."""
        return self.code.reshape(1, 1, 1, -1).repeat(1, self.channels, self.height, self.tiles)


class SPADELayer(nn.Module):
    """_init_spade.py:114-139: out = InstanceNorm(x) * (1 + gamma(F_id)) + beta(F_id), F_id resized to x by nearest neighbour.
    The parameter-free norm and the activation of the reference's module tree hold no state and are not modules here: they are the
    fused kernel's ``eps`` and ``slope``."""
    HIDDEN = 128
    EPS = 1e-5          # nn.InstanceNorm2d's default, which the reference uses

    def __init__(self, norm_nc, label_nc):
        super().__init__()
        self.mlp_shared = nn.Sequential(_conv3(label_nc, self.HIDDEN), nn.ReLU())
        self.conv_gamma, self.conv_beta = _conv3(self.HIDDEN, norm_nc), _conv3(self.HIDDEN, norm_nc)

    def forward(self, x, F_id, _slope=1.0):
        """_slope (not in the reference): the LeakyReLU slope of the SPADEBlock that follows, fused into the modulate kernel."""
        F_id = F_id.nearest(x.shape[-2:]) if isinstance(F_id, TiledCodeMap) else F.interpolate(F_id, size=x.shape[-2:], mode="nearest")
        hidden = self.mlp_shared(F_id)
        return ops.spade_modulate(x, self.conv_gamma(hidden), self.conv_beta(hidden), eps=self.EPS, slope=_slope)


class SPADEBlock(nn.Module):
    """_init_spade.py:235-282: two SPADE -> LeakyReLU -> spectral-normalised conv stages plus a SPADE shortcut, optionally halving
    (average pool on the main branch, strided conv on the shortcut) or doubling (nearest upsample / transposed conv) the resolution
    between the stages.  Registration order = the reference's: it fixes both the state_dict key order and the order in which the
    initialisers draw from the global RNG (tests/test_spade.py regenerates the reference's seeded weights)."""
    SLOPE = 0.2

    def __init__(self, in_channels, out_channels, fid_channels, downsample=False, upsample=False):
        super().__init__()
        for tag, cin in (("1", in_channels), ("2", out_channels)):
            self.add_module("spade" + tag, SPADELayer(cin, fid_channels))
            conv = _conv3(cin, out_channels)
            self.add_module("conv" + tag, conv)
            self.add_module("conv%s_sn" % tag, spectral_norm(conv))      # the same module under a second name, as in the reference
        self.downsample, self.upsample = bool(downsample), bool(upsample)
        if self.downsample:
            self.residual_downsample = _conv3(in_channels, in_channels, stride=2)
        if self.upsample:
            self.residual_upsample = nn.ConvTranspose2d(in_channels, in_channels, 3, 2, 1, output_padding=1)
        self.spade_s = SPADELayer(in_channels, fid_channels)
        self.conv_s = spectral_norm(_conv3(in_channels, out_channels))

    def forward(self, x, fid):
        main = self.conv1_sn(self.spade1(x, fid, _slope=self.SLOPE))
        skip = x
        if self.downsample:
            main, skip = F.avg_pool2d(main, 2, 2), self.residual_downsample(skip)
        if self.upsample:
            main, skip = F.interpolate(main, scale_factor=2, mode="nearest"), self.residual_upsample(skip)
        main = self.conv2_sn(self.spade2(main, fid, _slope=self.SLOPE))
        return self.conv_s(self.spade_s(skip, fid, _slope=self.SLOPE)) + main


def _conv_bn_relu(cin, cout):
    return nn.Sequential(_conv3(cin, cout), nn.BatchNorm2d(cout), nn.ReLU())


def _stem():
    """conv 3 -> 64 at full resolution, then 2x average pool: the first layer of both the identity encoder and the refiner."""
    return nn.Sequential(_conv3(3, 64), nn.AvgPool2d(2, 2))


class ResBlock2d(nn.Module):
    """_init_spade.py:7-37 (the identity encoder's residual block; library convolutions and batch norm throughout).  As in the
    reference a non-downsampling block needs in_channels == out_channels, and a downsampling one does not use ``residual``."""

    def __init__(self, in_channels, out_channels, downsample=False):
        super().__init__()
        self.downsample = bool(downsample)
        self.initial = _conv_bn_relu(in_channels, out_channels)
        if self.downsample:
            self.downsample_layer = _conv3(in_channels, out_channels, stride=2)
            self.residual_downsample = _conv3(out_channels, out_channels, stride=2)
        self.residual = _conv_bn_relu(out_channels, out_channels)

    def forward(self, x):
        y = self.initial(x)
        return self.residual_downsample(y) + self.downsample_layer(x) if self.downsample else self.residual(y) + x


class IdEncoder(nn.Module):
    """_init_spade.py:185-204: the three identity feature maps (64, 128, 256 channels at 1/2, 1/4, 1/8 resolution) that modulate the refiner."""
    WIDTHS = (64, 128, 256)

    def __init__(self):
        super().__init__()
        self.layer1 = _stem()
        cin = self.WIDTHS[0]
        for i, cout in enumerate(self.WIDTHS):
            self.add_module("layer%d" % (i + 2), ResBlock2d(cin, cout, downsample=i > 0))
            cin = cout

    def forward(self, x):
        x, maps = self.layer1(x), []
        for i in range(len(self.WIDTHS)):
            x = getattr(self, "layer%d" % (i + 2))(x)
            maps.append(x)
        return tuple(maps)


class RefineNetwork(nn.Module):
    """_init_spade.py:284-312: stem, six SPADE blocks (down, down, same, up, up, up; block k is modulated by identity map PLAN[k][2]),
    conv to RGB."""
    #        (in, out, identity map, resample)
    PLAN = ((64, 64, 0, "down"), (64, 128, 1, "down"), (128, 256, 2, None), (256, 256, 2, "up"), (256, 128, 1, "up"), (128, 64, 0, "up"))

    def __init__(self, fid_channels1, fid_channels2, fid_channels3):
        super().__init__()
        fid_channels = (fid_channels1, fid_channels2, fid_channels3)
        self.layer1 = _stem()
        for k, (cin, cout, which, how) in enumerate(self.PLAN):
            self.add_module("layer%d" % (k + 2), SPADEBlock(cin, cout, fid_channels[which], downsample=how == "down", upsample=how == "up"))
        self.layer8 = _conv3(64, 3)

    def forward(self, x, fid1, fid2, fid3):
        fids = (fid1, fid2, fid3)
        x = self.layer1(x)
        for k, plan in enumerate(self.PLAN):
            x = getattr(self, "layer%d" % (k + 2))(x, fids[plan[2]])
        return self.layer8(x)


class Generator(nn.Module):
    """_init_spade.py:315-325: the Stage-II generator G(I_src, I_raw) of eval_get_texture_photo_audio.py:154 -- identity features of the
    source image modulate the refinement of the Stage-I render."""

    def __init__(self):
        super().__init__()
        self.idencoder = IdEncoder()
        self.refine_network = RefineNetwork(*IdEncoder.WIDTHS)

    def forward(self, I_src, I_raw):
        return self.refine_network(I_raw, *self.idencoder(I_src))


class AudioNet(nn.Module):
    """_init_spade.py:327-357, the Stage-II file's own audio encoder: four stride-2 Conv1d over the 16-frame window of 29 DeepSpeech features,
    LeakyReLU(0.02) after each; its ``encoder_fc1`` exists (it is in the checkpoints) but the forward returns the 64 convolution features."""
    CHANNELS = (29, 32, 32, 64, 64)

    def __init__(self, dim_aud=76, win_size=16):
        super().__init__()
        self.win_size, self.dim_aud = win_size, dim_aud
        convs = []
        for cin, cout in zip(self.CHANNELS[:-1], self.CHANNELS[1:]):
            convs += [nn.Conv1d(cin, cout, 3, 2, 1), nn.LeakyReLU(0.02)]
        self.encoder_conv = nn.Sequential(*convs)
        self.encoder_fc1 = nn.Sequential(nn.Linear(64, 64), nn.LeakyReLU(0.02), nn.Linear(64, dim_aud))

    def forward(self, x):
        half = self.win_size // 2
        return self.encoder_conv(x[:, 8 - half:8 + half, :].transpose(1, 2)).squeeze(-1)


class Generator_audio(nn.Module):
    """_init_spade.py:359-372: G(I_src, I_raw, audio window) of eval_get_texture_photo_audio.py:156 -- the deepest identity map is replaced by
    the audio code tiled over a 256 x 64 x 4096 map (TiledCodeMap: never materialised here; its ``nearest`` is an index, an expand and a
    copy, so the AudioNet trains through it)."""

    def __init__(self):
        super().__init__()
        self.idencoder = IdEncoder()
        self.refine_network = RefineNetwork(*IdEncoder.WIDTHS)
        self.AudioNet = AudioNet(76, 16)

    def forward(self, I_src, I_raw, driving_data):
        fid1, fid2, _ = self.idencoder(I_src)
        code = self.AudioNet(driving_data.unsqueeze(0))                       # (1, 64)
        return self.refine_network(I_raw, fid1, fid2, TiledCodeMap(code, IdEncoder.WIDTHS[2], 64, 64))


class _FusedSpectralNorm:
    """The ONE forward pre-hook fuse_spectral_norm_ leaves on a module: every spectral-normalised submodule's weight from
    ``ops.spectral_normalize`` -- two launches and one autograd node for all of them, sigma in fp32 whatever autocast says -- where
    torch's per-module hooks run ~14 launches and 6 nodes each.  ``entries``: (submodule, its key in _forward_pre_hooks, torch's hook)
    -- what unfuse_spectral_norm_ puts back.  It holds the submodules themselves, so a deepcopy of the hooked module (which copies this
    object with the same memo) drives the copy's submodules."""

    def __init__(self, entries):
        self.entries = entries

    def __call__(self, module, inputs):
        groups = {}      # torch's hook iterates when ITS module trains, with its own eps: one call per (training, eps) met -- usually one
        for m, _, hook in self.entries:
            groups.setdefault((m.training, hook.eps), []).append((m, hook.name))
        for (training, eps), group in groups.items():
            get = lambda suffix: [getattr(m, name + suffix) for m, name in group]
            for (m, name), weight in zip(group, ops.spectral_normalize(get("_orig"), get("_u"), get("_v"), training, eps=eps)):
                setattr(m, name, weight)


def _fused_hook_key(module):
    return next((k for k, hook in module._forward_pre_hooks.items() if isinstance(hook, _FusedSpectralNorm)), None)


def fuse_spectral_norm_(module):
    """Opt-in, in place: take torch's SpectralNorm forward pre-hooks off every submodule of ``module`` (each found once, under
    whatever names it is registered) and put one hook on ``module`` that normalises all their weights with the fused op before its
    forward.  Parameters, buffers, state_dict and load_state_dict are untouched -- weight_orig, weight_u, weight_v stay where torch put
    them, an optimiser built before stays valid -- and refine_step works as it is, with and without autocast_dtype.  Already fused, or
    nothing to fuse: returns ``module`` as it is.  Hooks with n_power_iterations != 1 or dim != 0 are refused before anything changes."""
    if _fused_hook_key(module) is not None:
        return module
    named = [(name, m, key, hook) for name, m in module.named_modules() for key, hook in m._forward_pre_hooks.items()
             if isinstance(hook, SpectralNorm)]
    for name, _, _, hook in named:
        if hook.n_power_iterations != 1 or hook.dim != 0:
            raise ValueError("fuse_spectral_norm_: %s has spectral norm with n_power_iterations=%d, dim=%d; the fused op is "
                             "n_power_iterations=1, dim=0" % (name or "the module itself", hook.n_power_iterations, hook.dim))
    if named:
        for _, m, key, _ in named:
            del m._forward_pre_hooks[key]
        module.register_forward_pre_hook(_FusedSpectralNorm([(m, key, hook) for _, m, key, hook in named]))
    return module


def unfuse_spectral_norm_(module):
    """Undo fuse_spectral_norm_: torch's hooks back on the submodules, the fused hook off ``module``.  Not fused: returns it as it is."""
    key = _fused_hook_key(module)
    if key is not None:
        for m, k, hook in module._forward_pre_hooks.pop(key).entries:
            m._forward_pre_hooks[k] = hook
    return module


def refine_learning_rate(cfg, epoch):
    """train_get_texture_photo.py:147-155: ``texture_refine.lr_G`` for the first ``texture_refine.epochs`` epochs, then linearly to zero
    over ``texture_refine.epochs_decay`` more (the caller sets it on the optimiser's parameter groups at the start of each epoch)."""
    t = cfg.texture_refine
    if epoch < t.epochs:
        return t.lr_G
    return t.lr_G / t.epochs_decay * (t.epochs + t.epochs_decay - epoch)


class RefineLoss:
    """A training objective for ``refine_step``: ``l2 * MSE + l1 * L1 + ssim * (1 - SSIM)`` between the clamped output and the target --
    what a refiner is scored on (metrics.score_frames: L1, PSNR, SSIM) -- as ONE fused, differentiable op with the clamp inside
    (ops.image_loss: two launches forward, one scaling backward, bit-reproducible).  ``RefineLoss()`` is the reference's objective,
    ``RefineLoss(1, 1)`` the l2 + l1 variant its audio loop keeps commented (train_get_texture_photo_audio.py:189-191).  Under
    autocast the generator's bf16 output is widened first; the op itself runs in fp32 outside autocast.
    ``lpips > 0`` adds ``lpips * lpips_model.loss(fake, target, clamp=True)``, the fourth figure frames are scored on, with
    ``lpips_model`` a ``metrics.LPIPS`` object built from the user's weight files (metrics.LPIPS.loss: fused ends, the vendor
    library's convolutions between them); asking for it without a model is a ValueError.  With ``lpips == 0`` nothing changes."""

    def __init__(self, l2=1.0, l1=0.0, ssim=0.0, ssim_data_range=1.0, lpips=0.0, lpips_model=None):
        self.l2, self.l1, self.ssim, self.ssim_data_range = float(l2), float(l1), float(ssim), float(ssim_data_range)
        self.lpips, self.lpips_model = float(lpips), lpips_model
        if self.lpips > 0.0 and lpips_model is None:
            raise ValueError("RefineLoss: lpips = %g needs lpips_model, a metrics.LPIPS object (its weights do not ship here)" % self.lpips)

    def __call__(self, fake, target):
        fake = fake.float()
        loss = ops.image_loss(fake, target, l2=self.l2, l1=self.l1, ssim=self.ssim, clamp=True, ssim_data_range=self.ssim_data_range)
        if self.lpips > 0.0:
            loss = loss + self.lpips * self.lpips_model.loss(fake, target, clamp=True)
        return loss

    def __repr__(self):
        text = "RefineLoss(l2=%g, l1=%g, ssim=%g, ssim_data_range=%g" % (self.l2, self.l1, self.ssim, self.ssim_data_range)
        return text + (", lpips=%g)" % self.lpips if self.lpips > 0.0 else ")")


def refine_step(G, optimizer, I_src, I_raw, target, driving=None, loss=None, autocast_dtype=None):
    """One training step of the Stage-II generator, train_get_texture_photo.py:168-179 (``driving`` = the audio window of
    train_get_texture_photo_audio.py:143-192 for Generator_audio): MSE between the clamped output and the target frame, backward,
    optimiser step.  Returns the loss (a 0-d tensor; no synchronisation here).  The caller does ``G.train()``, the data loading and the
    learning-rate schedule, as with training.train_step.
    loss=None is the reference's objective in torch's own ops; a ``RefineLoss`` takes the place of the clamp and the MSE with its
    weighted MSE / L1 / SSIM objective, and nothing else in the step changes (any callable ``(fake, target) -> 0-d loss`` is taken).
    autocast_dtype=torch.bfloat16 (not in the reference): the generator's forward and the loss run under
    ``torch.autocast("cuda", dtype=torch.bfloat16)`` -- the convolutions on the bf16 matrix pipe, the SPADE modulation on its bf16
    kernels -- while backward() and the optimiser step run outside it; the parameters and Adam's state stay fp32, and bf16 has fp32's
    exponent range, so there is no GradScaler."""
    if autocast_dtype not in (None, torch.bfloat16):
        raise ValueError("refine_step: autocast_dtype must be None or torch.bfloat16, got %r" % (autocast_dtype,))
    if loss is not None and not callable(loss):
        raise ValueError("refine_step: loss must be None or a callable (fake, target) -> loss such as RefineLoss, got %r "
                         "(autocast_dtype is passed by keyword)" % (loss,))
    optimizer.zero_grad()
    with contextlib.nullcontext() if autocast_dtype is None else torch.autocast("cuda", dtype=autocast_dtype):
        fake = G(I_src, I_raw) if driving is None else G(I_src, I_raw, driving)
        loss = F.mse_loss(fake.clamp(0, 1), target) if loss is None else loss(fake, target)
    loss.backward()
    optimizer.step()
    return loss.detach()


# ---- Stage-II inference: the generator frozen against one identity photo ----
def _normalised_weights(G):
    """Run every spectral-norm forward pre-hook in ``G`` once -- torch's on the submodules, or fuse_spectral_norm_'s on the module that
    carries it -- so that each hooked convolution's ``weight`` is what eval mode normalises it to (no power iteration: G is in eval)."""
    for m in G.modules():
        for hook in list(m._forward_pre_hooks.values()):
            if isinstance(hook, (SpectralNorm, _FusedSpectralNorm)):
                hook(m, ())


def _conv_copy(conv, dtype):
    """(weight, bias) of a convolution as detached copies in ``dtype`` -- the cast torch.autocast makes per call, made once."""
    return conv.weight.detach().to(dtype, copy=True), conv.bias.detach().to(dtype, copy=True)


def _tiled_code_maps(code, channels, size, tiles=64):
    """TiledCodeMap.nearest for a batch of codes (B, n) -> (B, channels, h, w): one map per frame, by the same index rule."""
    h, w = int(size[0]), int(size[1])
    cols = torch.from_numpy(TiledCodeMap._nearest_index(w, code.shape[1] * tiles) % code.shape[1]).to(code.device)
    return code[:, cols].reshape(code.shape[0], 1, 1, w).expand(code.shape[0], channels, h, w).contiguous()


class FrozenRefiner:
    """What ``freeze_identity`` returns: a Stage-II generator with everything that depends on the identity photo alone computed once.
    ``frozen(I_raw)`` / ``frozen(I_raw, driving)`` returns what ``G(I_src, I_raw[, driving])`` returns for I_raw (B, 3, H, W), running
    per frame only the stem, each block's own and resampling convolutions, the pooling, ``ops.spade_modulate_frozen`` and ``layer8``.
    A SNAPSHOT: it holds copies of the maps and of every weight it needs (spectral-normalised ones as eval mode normalises them), so
    later changes to ``G`` -- an optimiser step, load_state_dict -- are not seen; freeze again after changing G.  Inference only."""

    def __init__(self, size, dtype, fold_upsample, stem, blocks, layer8, audio):
        self.size, self.dtype, self.fold_upsample = tuple(size), dtype, bool(fold_upsample)
        self.stem, self.blocks, self.layer8, self.audio = stem, blocks, layer8, audio

    def _tensors(self, maps_only=False):
        for blk in self.blocks:
            for key in ("spade1", "spade2", "spade_s"):
                if blk[key][0] == "maps" or not maps_only:
                    yield from blk[key][1]
            if not maps_only:
                for key in ("conv1", "conv2", "conv_s", "resample"):
                    yield from blk[key] or ()
        if not maps_only:
            yield from self.stem + self.layer8
            for conv in self.audio or ():
                yield from conv

    @property
    def cached_map_bytes(self):
        """Bytes of the cached gamma / beta maps alone."""
        return sum(t.numel() * t.element_size() for t in self._tensors(maps_only=True))

    @property
    def cached_bytes(self):
        """Bytes of everything the snapshot holds: the gamma / beta maps and the weight copies."""
        return sum(t.numel() * t.element_size() for t in self._tensors())

    @property
    def device(self):
        return self.layer8[0].device

    def _modulate(self, layer, x, code, up=False):
        kind, tensors = layer
        if kind == "maps":
            gamma, beta = tensors
        else:      # a layer modulated by the audio code: its gamma / beta convolutions run per call, from one tiled map per code
            size = (2 * x.shape[2], 2 * x.shape[3]) if up else x.shape[2:]
            hidden = F.relu(F.conv2d(_tiled_code_maps(code, IdEncoder.WIDTHS[2], size), tensors[0], tensors[1], padding=1))
            gamma, beta = F.conv2d(hidden, tensors[2], tensors[3], padding=1), F.conv2d(hidden, tensors[4], tensors[5], padding=1)
        return ops.spade_modulate_frozen(x, gamma, beta, eps=SPADELayer.EPS, slope=SPADEBlock.SLOPE, up=up)

    def __call__(self, I_raw, driving=None):
        if I_raw.dim() != 4 or tuple(I_raw.shape[1:]) != (3,) + self.size:
            raise ValueError("FrozenRefiner: frozen for frames of (B, 3, %d, %d), got %s (freeze_identity(..., size=...) fixes the size "
                             "of the cached maps)" % (self.size + (tuple(I_raw.shape),)))
        if (driving is None) != (self.audio is None):
            raise ValueError("FrozenRefiner: a Generator_audio snapshot takes driving (16, 29) or (B, 16, 29), a Generator snapshot none")
        with torch.no_grad():
            code = None
            if driving is not None:
                if driving.shape[-2:] != (16, 29) or driving.dim() not in (2, 3) or (driving.dim() == 3 and driving.shape[0] != I_raw.shape[0]):
                    raise ValueError("FrozenRefiner: driving must be (16, 29) or (%d, 16, 29), got %s" % (I_raw.shape[0], tuple(driving.shape)))
                code = (driving if driving.dim() == 3 else driving.unsqueeze(0)).to(self.dtype)
                code = code.transpose(1, 2)      # (AudioNet.forward's window 8 - 16 // 2 : 8 + 16 // 2 is all 16 rows)
                for weight, bias in self.audio:
                    code = F.leaky_relu(F.conv1d(code, weight, bias, stride=2, padding=1), 0.02)
                code = code.squeeze(-1)
            x = F.avg_pool2d(F.conv2d(I_raw.to(self.dtype), self.stem[0], self.stem[1], padding=1), 2, 2)
            for blk in self.blocks:
                main = F.conv2d(self._modulate(blk["spade1"], x, code), blk["conv1"][0], blk["conv1"][1], padding=1)
                skip, fold = x, False
                if blk["how"] == "down":
                    main, skip = F.avg_pool2d(main, 2, 2), F.conv2d(skip, blk["resample"][0], blk["resample"][1], stride=2, padding=1)
                if blk["how"] == "up":
                    skip = F.conv_transpose2d(skip, blk["resample"][0], blk["resample"][1], stride=2, padding=1, output_padding=1)
                    fold = self.fold_upsample
                    if not fold:
                        main = F.interpolate(main, scale_factor=2, mode="nearest")
                main = F.conv2d(self._modulate(blk["spade2"], main, code, up=fold), blk["conv2"][0], blk["conv2"][1], padding=1)
                x = F.conv2d(self._modulate(blk["spade_s"], skip, code), blk["conv_s"][0], blk["conv_s"][1], padding=1) + main
            y = F.conv2d(x, self.layer8[0], self.layer8[1], padding=1)
        return y.float() if self.dtype == torch.bfloat16 else y


def freeze_identity(G, I_src, size=None, dtype=torch.float32, fold_upsample=True):
    """Freeze a Generator or Generator_audio against the identity photo ``I_src`` (1, 3, H, W) -> a ``FrozenRefiner`` for frames of
    ``size`` (H, W) (default: the photo's).  Computed ONCE here, under no_grad: the identity maps and, for every SPADE layer they feed,
    gamma and beta at that layer's own resolution; every convolution weight of the per-frame path, spectral-normalised ones as eval
    mode normalises them (torch's hooks or fuse_spectral_norm_'s).  For Generator that is 75 % of the forward's multiply-adds; for
    Generator_audio the layers modulated by the audio code keep their gamma / beta convolutions per call.
    ``G`` must be in eval mode (batch norm's batch statistics and spectral norm's power iteration would make the snapshot wrong).  The
    result is a copy: it does not follow later changes to ``G``.
    dtype=torch.bfloat16: maps and weights are computed as ``G`` under ``torch.autocast(device, torch.bfloat16)`` computes them and
    stored in bf16; the per-frame path then runs on bf16 tensors with no per-call casts and returns float32.  torch.float64 is taken
    too (with ``G.double()``: the host tests).
    fold_upsample: the nearest 2x upsample of the three "up" blocks is read in place by the modulation (``up=True``) instead of
    written out by F.interpolate."""
    if dtype not in (torch.float32, torch.bfloat16, torch.float64):
        raise ValueError("freeze_identity: dtype must be torch.float32, torch.bfloat16 or torch.float64, got %r" % (dtype,))
    if not isinstance(G, (Generator, Generator_audio)):
        raise ValueError("freeze_identity: G must be a Generator or a Generator_audio, got %s" % type(G).__name__)
    if any(m.training for m in G.modules()):
        raise ValueError("freeze_identity: G must be in eval mode (call G.eval()): batch norm's batch statistics and spectral norm's "
                         "power iteration would make the snapshot wrong")
    if I_src.dim() != 4 or I_src.shape[0] != 1 or I_src.shape[1] != 3:
        raise ValueError("freeze_identity: I_src must be (1, 3, H, W), got %s" % (tuple(I_src.shape),))
    size = tuple(int(s) for s in (I_src.shape[2:] if size is None else size))
    audio = isinstance(G, Generator_audio)
    autocast = torch.autocast(I_src.device.type, dtype=torch.bfloat16) if dtype == torch.bfloat16 else contextlib.nullcontext()
    net = G.refine_network
    with torch.no_grad(), autocast:
        _normalised_weights(G)
        fids = G.idencoder(I_src)

        def layer_state(layer, which, res):
            if audio and which == 2:
                return ("audio", _conv_copy(layer.mlp_shared[0], dtype) + _conv_copy(layer.conv_gamma, dtype) + _conv_copy(layer.conv_beta, dtype))
            hidden = layer.mlp_shared(F.interpolate(fids[which], size=res, mode="nearest"))
            return ("maps", (layer.conv_gamma(hidden).to(dtype, copy=True), layer.conv_beta(hidden).to(dtype, copy=True)))

        res, blocks = (size[0] // 2, size[1] // 2), []
        for k, (_, _, which, how) in enumerate(RefineNetwork.PLAN):
            block = getattr(net, "layer%d" % (k + 2))
            after = {"down": (res[0] // 2, res[1] // 2), "up": (2 * res[0], 2 * res[1]), None: res}[how]
            resample = {"down": getattr(block, "residual_downsample", None), "up": getattr(block, "residual_upsample", None), None: None}[how]
            blocks.append(dict(how=how, spade1=layer_state(block.spade1, which, res), spade2=layer_state(block.spade2, which, after),
                               spade_s=layer_state(block.spade_s, which, after), conv1=_conv_copy(block.conv1_sn, dtype),
                               conv2=_conv_copy(block.conv2_sn, dtype), conv_s=_conv_copy(block.conv_s, dtype),
                               resample=None if resample is None else _conv_copy(resample, dtype)))
            res = after
        audio_convs = [_conv_copy(m, dtype) for m in G.AudioNet.encoder_conv if isinstance(m, nn.Conv1d)] if audio else None
        return FrozenRefiner(size, dtype, fold_upsample, _conv_copy(net.layer1[0], dtype), blocks, _conv_copy(net.layer8, dtype), audio_convs)


def _frame_bytes(frame, device, quantise):
    """One frame of refine_frames' input -> (H, W, 3) uint8, or float as it is with quantise=False, on ``device``."""
    frame = torch.as_tensor(frame).to(device)
    if frame.dim() != 3 or frame.shape[2] != 3:
        raise ValueError("refine_frames: a frame must be (H, W, 3), got %s" % (tuple(frame.shape),))
    if frame.dtype == torch.uint8 or (not quantise and frame.is_floating_point()):
        return frame
    if frame.is_floating_point():
        return (frame.clamp(0.0, 1.0) * 255).to(torch.uint8)      # evaluation.cast_to_image: what the PNG between the stages holds
    raise ValueError("refine_frames: frames are uint8 or float (H, W, 3), got %s" % frame.dtype)


def refine_frames(frozen, frames, driving=None, batch=8, quantise=True, savedir=None, log=print):
    """The Stage-II evaluation loop (eval_get_texture_photo.py / eval_get_texture_photo_audio.py): every Stage-I frame through the frozen
    generator, clipped, x255, truncated to bytes -> the list of (H, W, 3) uint8 tensors on the frozen model's device, also written as
    ``f_%04d.png`` (numbered from 0) under ``savedir`` when given.
    frames: an iterable (a generator works) of (H, W, 3) uint8 arrays or tensors, on any device -- a PNG's content, or
    ``render_frames(..., fused_products=True)[i]["bytes"]["image"]`` -- or float (H, W, 3) tensors in [0, 1]; those go through the
    cast_to_image rule first when ``quantise`` (the reference always reads a PNG), and are fed as they are otherwise.  Bytes become
    the reference's input: / 255 in float32, CHW.  driving: a sequence of (16, 29) audio windows, one per frame, for a
    Generator_audio snapshot.  Up to ``batch`` frames go through ``frozen`` per call."""
    from .evaluation import _save_png
    batch, out, n = max(int(batch), 1), [], 0
    windows = None if driving is None else iter(driving)

    def flush(chunk):
        nonlocal n
        x = torch.stack([f.to(torch.float32) / 255 if f.dtype == torch.uint8 else f.to(torch.float32) for f in chunk]).permute(0, 3, 1, 2)
        d = None if windows is None else torch.stack([torch.as_tensor(next(windows)).to(frozen.device) for _ in chunk])
        y = frozen(x.contiguous()) if d is None else frozen(x.contiguous(), d)
        for img in (y.clamp(0.0, 1.0) * 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous():
            if savedir is not None:
                _save_png(os.path.join(savedir, "f_%04d.png" % n), img.cpu().numpy())
            out.append(img)
            n += 1

    chunk = []
    for frame in frames:
        chunk.append(_frame_bytes(frame, frozen.device, quantise))
        if len(chunk) == batch:
            flush(chunk)
            chunk = []
    if chunk:
        flush(chunk)
    if log is not None:
        log("refine_frames: %d frames%s" % (n, "" if savedir is None else " -> " + str(savedir)))
    return out
