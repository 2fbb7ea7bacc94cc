"""Stage-I training step around the HIP ops (BASELINE.json configs[4]; semantics of
``train_stage_rays_auto.py:390-509``, which is out of sync with ``nerf/`` as shipped -- SURVEY.md section 0.3 -- so this
mirrors what the step computes, not its tuple unpacking).

  1. semantic-weighted ray sampling: p(pixel) ~ sum_c sample_prob[c] * mask[pixel, c]            (:390-394, :417-419)
  2. 2048 rays without replacement; gather origins, directions, target colour, background prior, class mask (:421-432)
  3. run_one_iter_of_nerf(mode="train") -> coarse and fine 15-channel renders                               (:437-452)
  4. loss = sum over {coarse, fine} of  MSE + 0.02 * CE + 0.005 * (masked MSE + masked CE of classes 7:9)   (:455-465)
     [+ 0.005 * ||spatial_embeddings|| when regularize_spatial_embedding]                                  (:476-477, :490-491)
  5. sample_prob <- normalised sum of the four weighted per-class losses (feeds the next step's sampling)   (:466-468)
  6. backward, Adam step, lr = lr0 * decay_factor ** (i / (lr_decay * 1000))                               (:493-509)
"""
import torch

from .nerf_helpers import MaskCrossEntropyLoss, MaskMSELoss, get_ray_bundle, mse2psnr
from .train_utils import run_one_iter_of_nerf


def semantic_ray_probs(sample_prob, mask):
    """(12,), (H, W, 12) -> (H*W,) sampling distribution over pixels."""
    p = torch.sum(sample_prob.reshape(1, 1, -1) * mask, dim=-1).reshape(-1).double()
    return (p / p.sum()).float()


def sample_training_rays(probs, num_rays, generator=None):
    """Indices of ``num_rays`` distinct pixels drawn with probability ``probs`` (np.random.choice(replace=False, p=...))."""
    return torch.multinomial(probs, num_rays, replacement=False, generator=generator)


def sample_prob_weights(device=None, dtype=torch.float32):
    """train_stage_rays_auto.py:268-269: the per-class weights both loss modules are built with -- ones(12) with the mouth
    classes 7 and 8 doubled.  They do not enter the loss value, only the weighted per-class losses that become the next
    step's sampling distribution (:466-468)."""
    w = torch.ones(12, device=device, dtype=dtype)
    w[7:9] = 2
    return w


def stage1_loss(rgb_coarse, rgb_fine, target_rgb, mask, mse_loss=None, ce_loss=None):
    """train_stage_rays_auto.py:455-468 -> (loss, new_sample_prob, fine_mse).  rgb_*: (R,15) = [rgb3 | seg12]; target_rgb (R,3);
    mask (R,12) one-hot.  The loss modules default to the script's own (:270-271: weights ones(12), [7:9] = 2)."""
    if mse_loss is None:
        mse_loss = MaskMSELoss(sample_prob_weights(mask.device, rgb_coarse.dtype))
    if ce_loss is None:
        ce_loss = MaskCrossEntropyLoss(sample_prob_weights(mask.device, rgb_coarse.dtype))
    total, weighted = 0.0, []
    fine_mse = None
    for rgb in (rgb_coarse, rgb_fine):
        if rgb is None:
            continue
        l2, m_l2, m_l2_w = mse_loss(mask, rgb[..., :3], target_rgb[..., :3])
        ce, m_ce, m_ce_w = ce_loss(mask, rgb[..., 3:], mask)
        mouth = torch.sum(m_l2[7:9] + m_ce[7:9])
        total = total + l2 + 0.02 * ce + 0.005 * mouth
        weighted += [m_l2_w, m_ce_w]
        fine_mse = l2
    w = torch.stack([x.detach() for x in weighted]).sum(0)
    return total, w / w.sum(), fine_mse


def learning_rate(cfg, step):
    return cfg.optimizer.lr * (cfg.scheduler.lr_decay_factor ** (step / (cfg.scheduler.lr_decay * 1000)))


def train_step(model, optimizer, cfg, step, image, mask, pose, intrinsics, audio, background, sample_prob, generator=None,
               regularize_spatial_embedding=False, group=None, fused_loss=True):
    """One optimisation step on one frame.  image (H,W,3), mask (H,W,12) one-hot float, background (H,W,15).
    Returns dict(loss, psnr, sample_prob).

    Under torch.distributed (one process per GPU) the step is data-parallel over rays: every rank draws the same batch
    (``generator`` seeded identically), renders and back-propagates its contiguous slice, and the gradients -- and the
    per-class sampling feedback -- are averaged with one all-reduce each before the optimiser step, so the replicas stay
    identical.

    fused_loss: the objective is evaluated by one HIP launch on the rendered maps and its gradient is formed inside the composite
    backward kernels (ops.RenderRaysFn with loss operands) instead of ~40 small torch kernels and an (R,15) gradient round trip;
    same recipe, same class weights (stage1_loss is the unfused statement, kept for the seams and the tests)."""
    import torch.distributed as dist
    from . import distributed as D
    H, W = image.shape[:2]
    probs = semantic_ray_probs(sample_prob, mask)
    sel = sample_training_rays(probs, int(cfg.nerf.train.num_random_rays), generator)
    sel = sel[D.shard_batch(sel.shape[0], group)]
    ro, rd = get_ray_bundle(H, W, intrinsics, pose)
    ro, rd = ro.reshape(-1, 3)[sel], rd.reshape(-1, 3)[sel]
    target = image.reshape(-1, image.shape[-1])[sel]
    bg = background.reshape(-1, 15)[sel] if background is not None else None
    m = mask.reshape(-1, 12)[sel].float()
    if fused_loss and m.is_cuda and sel.shape[0] <= int(cfg.nerf.train.chunksize):
        outs = run_one_iter_of_nerf(H, W, intrinsics, model, ro, rd, cfg, mode="train", driving=audio, pose=pose, background_prior=bg, inHead=m,
                                    _loss=(target[..., :3].float(), m, sample_prob_weights(m.device)))
        loss, stats = outs[8], outs[9]
        new_prob, fine_mse = stats[2:14].clone(), stats[1].clone()
    else:
        outs = run_one_iter_of_nerf(H, W, intrinsics, model, ro, rd, cfg, mode="train", driving=audio, pose=pose, background_prior=bg, inHead=m)
        loss, new_prob, fine_mse = stage1_loss(outs[0], outs[3], target, m)
    if regularize_spatial_embedding:
        loss = loss + torch.norm(model.spatial_embeddings) * 0.0005 * 10
    optimizer.zero_grad(set_to_none=True)
    loss.backward()
    if dist.is_initialized() and dist.get_world_size(group) > 1:
        if getattr(optimizer, "flat_grad", None) is not None:      # FlatAdam: the gradients are one buffer, averaged as the kernel reads them
            optimizer.grad_scale = D.all_reduce_flat_gradient(optimizer.flat_grad, group)
        else:
            D.all_reduce_gradients(model.parameters(), group)
        stats = torch.cat([new_prob, loss.detach().reshape(1), fine_mse.detach().reshape(1)])
        dist.all_reduce(stats, group=group)
        stats /= dist.get_world_size(group)
        new_prob, loss, fine_mse = stats[:-2] / stats[:-2].sum(), stats[-2], stats[-1]
    optimizer.step()
    for param_group in optimizer.param_groups:
        param_group["lr"] = learning_rate(cfg, step)
    return dict(loss=float(loss.detach()), psnr=mse2psnr(float(fine_mse.detach())), sample_prob=new_prob)


class FlatAdam:
    """torch.optim.Adam (weight_decay 0, no amsgrad: what the reference builds, train_stage_rays_auto.py:201-209) for a model whose
    parameters are one flat buffer (model.flatten_parameters_()): step() is ONE HIP launch over that buffer (ops.adam_step) instead of
    torch's per-tensor kernels, and zero_grad() one memset of the flat gradient buffer.  Drop-in where train_step and the checkpoint
    functions use an optimiser: param_groups[0]["lr"] is read at every step, and state_dict() / load_state_dict() speak
    torch.optim.Adam's format (per-parameter step / exp_avg / exp_avg_sq), so a checkpoint written with either loads into the other."""

    def __init__(self, model, lr, betas=(0.9, 0.999), eps=1e-8):
        if getattr(model, "_flat", None) is None:
            raise ValueError("FlatAdam needs a flattened model: call model.flatten_parameters_() first")
        self.model = model
        params = list(model._flat_params)
        if any(not p.requires_grad for p in params):
            raise ValueError("FlatAdam trains every parameter of the model")
        # the param-group keys (and their defaults) of the installed torch
        group = torch.optim.Adam([torch.zeros(1)], lr=lr, betas=betas, eps=eps).state_dict()["param_groups"][0]
        self.param_groups = [dict(group, params=params)]
        self.exp_avg = torch.zeros_like(model._flat)
        self.exp_avg_sq = torch.zeros_like(model._flat)
        self._step = 0
        self.grad_scale = 1.0      # train_step sets 1 / world after its summed all-reduce of flat_grad

    @property
    def flat_grad(self):
        return self.model._flat_grad

    def _group(self):
        if len(self.param_groups) != 1:
            raise NotImplementedError("FlatAdam has one param group (the reference's train_background groups are not covered)")
        g = self.param_groups[0]
        if g.get("weight_decay", 0) != 0 or g.get("amsgrad", False) or g.get("maximize", False):
            raise NotImplementedError("FlatAdam is plain Adam: weight_decay = 0, amsgrad = False, maximize = False")
        return g

    def zero_grad(self, set_to_none=True):
        """One memset; the parameters' .grad stay views of the flat gradient buffer whatever set_to_none says."""
        self.model._flat_grad.zero_()

    @torch.no_grad()
    def step(self, closure=None):
        from . import ops
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        g, m = self._group(), self.model
        if m._flat is None or m._flat.numel() != self.exp_avg.numel() or m._flat.device != self.exp_avg.device:
            raise RuntimeError("the model left flat mode or moved to another device since this optimiser was built")
        self._step += 1
        ops.adam_step(m._flat, m._flat_grad, self.exp_avg, self.exp_avg_sq, lr=g["lr"], beta1=g["betas"][0], beta2=g["betas"][1], eps=g["eps"],
                      step=self._step, grad_scale=self.grad_scale)
        m._flat_epoch += 1      # the kernel wrote the parameters through a raw pointer: model.packed() must re-pack
        return loss

    def _views(self, flat):
        out, off = [], 0
        for p in self.model._flat_params:
            out.append(flat[off:off + p.numel()].view(p.shape))
            off += p.numel()
        return out

    def state_dict(self):
        g = self._group()
        n = len(g["params"])
        state = {}
        if self._step > 0:
            for i, (a, b) in enumerate(zip(self._views(self.exp_avg), self._views(self.exp_avg_sq))):
                state[i] = {"step": torch.tensor(float(self._step)), "exp_avg": a, "exp_avg_sq": b}
        return {"state": state, "param_groups": [dict({k: v for k, v in g.items() if k != "params"}, params=list(range(n)))]}

    def load_state_dict(self, state_dict):
        groups = state_dict["param_groups"]
        if len(groups) != 1:
            raise NotImplementedError("FlatAdam has one param group")
        params = self.param_groups[0]["params"]
        if len(groups[0]["params"]) != len(params):
            raise ValueError("the optimiser state covers %d parameters, the model has %d" % (len(groups[0]["params"]), len(params)))
        state = state_dict["state"]
        steps = {int(s["step"]) for s in state.values()}
        if state and (len(state) != len(params) or len(steps) != 1):
            raise ValueError("FlatAdam keeps one step count for all parameters: the state must cover every parameter at the same step")
        old = self.param_groups
        self.param_groups = [dict({k: (tuple(v) if k == "betas" else v) for k, v in groups[0].items() if k != "params"}, params=params)]
        try:
            self._group()
        except NotImplementedError:
            self.param_groups = old
            raise
        with torch.no_grad():
            if not state:
                self._step = 0
                self.exp_avg.zero_()
                self.exp_avg_sq.zero_()
                return
            for idx, a, b in zip(groups[0]["params"], self._views(self.exp_avg), self._views(self.exp_avg_sq)):
                s = state[idx]
                a.copy_(s["exp_avg"])
                b.copy_(s["exp_avg_sq"])
            self._step = steps.pop()


def save_checkpoint(path, step, model, optimizer, loss, i_batch=0, background=None, latent_codes=None, pose_c=None, sample_prob=None):
    """The checkpoint dict of train_stage_rays_auto.py:698-722 (same keys), so files written here load in the reference and
    vice versa (its eval script reads model_state_dict / background / pose_c, eval_stage_rays.py:302-327)."""
    torch.save({"iter": int(step), "i_batch": int(i_batch), "model_state_dict": model.state_dict(),
                "optimizer_state_dict": optimizer.state_dict(), "loss": float(loss),
                "background": None if background is None else background.detach().clone(),
                "latent_codes": None if latent_codes is None else latent_codes.detach().clone(),
                "pose_c": pose_c, "sample_prob": None if sample_prob is None else sample_prob.detach().clone()}, path)


def resume(path, model, optimizer, device):
    """train_stage_rays_auto.py:238-258: -> dict(start_iter, i_batch, background, latent_codes, sample_prob).  weights_only load."""
    ck = torch.load(path, map_location=device, weights_only=True)
    model.load_state_dict(ck["model_state_dict"])
    optimizer.load_state_dict(ck["optimizer_state_dict"])
    return dict(start_iter=int(ck["iter"]) + 1, i_batch=int(ck.get("i_batch", 0)), background=ck.get("background"),
                latent_codes=ck.get("latent_codes"), sample_prob=ck.get("sample_prob"), pose_c=ck.get("pose_c"))
