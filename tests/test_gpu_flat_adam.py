"""The one-launch optimiser step on the MI355X: ops.adam_step against torch.optim.Adam in float64 (held to torch's own fp32 error: the
project's yardstick, conftest.yardstick), training.FlatAdam inside training.train_step on a flattened model -- gradient routing, offsets
and schedule pinned by replaying the captured gradients through torch.optim.Adam --, the packed weight streams never stale, checkpoints
interchangeable with torch.optim.Adam's, and two data-parallel ranks reducing the one flat gradient buffer."""
import os
import sys
import time

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import REPO, free_port, pkg, yardstick

pytestmark = pytest.mark.gpu

ARCHS = ("audio", "nerface", "nerface_static")
CFG = {"audio": "audio", "nerface": "expression", "nerface_static": "expression_static"}


def dev():
    return torch.device("cuda:0")


# ---- 1. the update arithmetic ---------------------------------------------------------------------------------------------------------
def _gradient(kind, n, k, seed):
    """Seeded and finite.  wide: magnitudes over eight orders with 5 % exact zeros; uniform: one scale."""
    g = torch.Generator(device=dev()).manual_seed(1000 * seed + k)
    x = torch.randn(n, device=dev(), generator=g)
    if kind == "uniform":
        return x * 1e-3
    x = x * 10.0 ** (torch.rand(n, device=dev(), generator=g) * 8.0 - 6.0)
    return x * (torch.rand(n, device=dev(), generator=g) >= 0.05)


def _param_counts():
    L = pkg("_lib").lib()
    return [int(L.sahs_model_param_count(m)) for m in (0, 1, 2)]


# (n, offset of params, offset of the other three buffers) in floats from a 16-byte boundary: 0/0 and 1/1 take the 16-byte path (with a
# scalar head for 1/1), 1/0 the element-by-element one
SMALL = [(n, a, b) for n in (1, 3, 4, 5, 1023, 1025) for a, b in ((0, 0), (1, 1), (1, 0))]


def _adam_case(n, off_p, off_o, kind, K=50):
    ops, Tr, sahs = pkg("ops"), pkg("training"), pkg()
    cfg = sahs.default_config()
    g0 = torch.Generator(device=dev()).manual_seed(n % 9973)
    start = torch.randn(n, device=dev(), generator=g0) * 0.2
    bufs = [torch.zeros(n + 8, device=dev()) for _ in range(4)]
    p, g, m, v = (b[o:o + n] for b, o in zip(bufs, (off_p, off_o, off_o, off_o)))
    assert p.data_ptr() % 16 == 4 * off_p and m.data_ptr() % 16 == 4 * off_o
    p.copy_(start)
    t32, t64 = start.clone().requires_grad_(True), start.double().requires_grad_(True)
    o32, o64 = (torch.optim.Adam([t], lr=1.0, foreach=False) for t in (t32, t64))
    for k in range(K):
        lr = Tr.learning_rate(cfg, 1000 * k)      # a different value at every step
        gk = _gradient(kind, n, k, n % 9973)
        t32.grad, t64.grad = gk.clone(), gk.double()
        for o in (o32, o64):
            o.param_groups[0]["lr"] = lr
            o.step()
        g.copy_(gk)
        ops.adam_step(p, g, m, v, lr=lr, step=k + 1)
    torch.cuda.synchronize()
    for b, o in zip(bufs, (off_p, off_o, off_o, off_o)):      # nothing outside [o, o + n) was written
        assert not bool(b[:o].any()) and not bool(b[o + n:].any())
    tag = "adam_step n=%d off=%d/%d %s: " % (n, off_p, off_o, kind)
    s32, s64 = o32.state[t32], o64.state[t64]
    for name, got, r32, r64 in (("params", p, t32, t64), ("exp_avg", m, s32["exp_avg"], s64["exp_avg"]),
                                ("exp_avg_sq", v, s32["exp_avg_sq"], s64["exp_avg_sq"])):
        r32, r64 = r32.detach().cpu().numpy(), r64.detach().cpu().numpy()
        assert np.isfinite(r64).all(), tag + name
        if n >= 1023:      # torch's own fp32 error is not zero: the yardstick is not degenerate
            assert np.abs(r32.astype(np.float64) - r64).max() > 0.0, tag + name
        yardstick(got, r32, r64, tag + name)


@pytest.mark.parametrize("kind", ["wide", "uniform"])
@pytest.mark.parametrize("n,off_p,off_o", SMALL)
def test_adam_step_vs_float64_small(n, off_p, off_o, kind):
    _adam_case(n, off_p, off_o, kind)


@pytest.mark.parametrize("kind", ["wide", "uniform"])
@pytest.mark.parametrize("model", [0, 1, 2])
def test_adam_step_vs_float64_model_sizes(model, kind):
    """50 consecutive updates of a buffer of each model's parameter count, a new learning rate at every step; params, exp_avg and
    exp_avg_sq within 2 x (rms) / 3 x (max) of torch's own fp32 error against torch.optim.Adam in float64, + 32 ulps of the tensor's
    scale; every element counted.  The audio model's count (2,775,633, odd) also from a base pointer one float off a 16-byte boundary."""
    n = _param_counts()[model]
    _adam_case(n, 0, 0, kind)
    if model == 0:
        _adam_case(n, 1, 1, kind)


# ---- the training scene of test_training_loop_reduces_loss, for every architecture -----------------------------------------------------
def _scene(arch, rays=512):
    sahs, W = pkg(), pkg("weights")
    cfg = sahs.default_config() if arch == "audio" else sahs.default_config(CFG[arch])
    cfg.nerf.train.num_random_rays = rays
    fw = W.flatten_state_dict(W.hash_state_dict(0, 8.0, 30.0, model=arch), model=arch)
    g = torch.Generator(device=dev()).manual_seed(0)
    H = Wd = 32
    image = torch.rand(H, Wd, 3, device=dev(), generator=g) * 0.2 + 0.4
    mask = torch.zeros(H, Wd, 12, device=dev())
    mask[..., 0] = 1.0
    mask[8:16, 8:16] = 0.0
    mask[8:16, 8:16, 7] = 1.0
    bgp = torch.cat([torch.rand(H, Wd, 3, device=dev(), generator=g), torch.ones(H, Wd, 1, device=dev()), torch.zeros(H, Wd, 11, device=dev())], -1)
    drv = torch.randn(16, 29, device=dev(), generator=g) if arch == "audio" else torch.randn(76, device=dev(), generator=g) * 0.5
    pose = torch.from_numpy(np.concatenate([np.eye(3), [[0.0], [0.0], [0.8 if arch == "audio" else 0.5]]], 1).astype(np.float32)).to(dev())
    intr = np.array([1200.0 * H / 512, 1200.0 * H / 512, 0.5, 0.5], np.float32)

    def model():
        cls = sahs.AudioFaceModel if arch == "audio" else sahs.NeRFaceModel
        return cls(cfg).to(dev()).load_flat(fw).train()

    return dict(cfg=cfg, fw=fw, model=model, args=(image, mask, pose, intr, drv, bgp), H=H, pose=pose, intr=intr, drv=drv, bgp=bgp)


def _capturing(opt, model):
    """Wrap opt.step: a clone of the flat gradient, the learning rate and the gradient scale in force right before every update."""
    caps, inner = [], opt.step

    def step():
        caps.append((model._flat_grad.clone(), float(opt.param_groups[0]["lr"]), float(opt.grad_scale)))
        return inner()

    opt.step = step
    return caps


def _replay(scene, caps, lr0):
    """The captured gradients through torch.optim.Adam(foreach=False) on unflattened copies with the same initial weights, in fp32 and
    in float64 -> the two flat parameter vectors (numpy)."""
    out = []
    for dtype in (torch.float32, torch.float64):
        m = scene["model"]()
        if dtype == torch.float64:
            m = m.double()
        params = list(m.parameters())
        opt = torch.optim.Adam(params, lr=lr0, foreach=False)
        for grad, lr, scale in caps:
            off = 0
            for p in params:
                p.grad = (grad[off:off + p.numel()].to(dtype) * scale).view_as(p).clone()
                off += p.numel()
            opt.param_groups[0]["lr"] = lr
            opt.step()
        out.append(torch.cat([p.detach().reshape(-1) for p in params]).cpu().numpy())
    return out


_WRITTEN = {}


def _written_words(arch, prec, flat):
    """The words of a packed stream that the pack kernels write (the streams are padded to tile boundaries, and the padding of a fresh
    allocation is whatever the allocator hands out): packed twice over buffers pre-filled with all-zero and all-one bits, the written
    words are those that come out equal."""
    if (arch, prec) not in _WRITTEN:
        L, ops = pkg("_lib").lib(), pkg("ops")
        words = int(L.sahs_model_packed_words(ARCHS.index(arch), prec))
        a, b = torch.zeros(words, dtype=torch.int32, device=dev()), torch.full((words,), -1, dtype=torch.int32, device=dev())
        torch.cuda.synchronize()
        for t in (a, b):
            assert L.sahs_model_pack_weights(ARCHS.index(arch), flat.data_ptr(), t.data_ptr(), prec, ops._stream()) == 0
        torch.cuda.synchronize()
        _WRITTEN[arch, prec] = a == b
        assert int(_WRITTEN[arch, prec].sum()) >= flat.numel() // 2
    return _WRITTEN[arch, prec]


def _assert_fresh(model, what):
    """packed() of every cached precision is, bit for bit, the pack of the buffer as it is now (every word the pack kernels write), and
    a second call re-packs nothing"""
    ops = pkg("ops")
    for prec in (ops.SAHS_F32, ops.SAHS_BF16X3):
        got = model.packed(prec)[0]
        want = ops.pack_weights(model.flat_params().clone(), prec, arch=model.arch)
        mask = _written_words(model.arch, prec, model.flat_params())
        assert got.shape == want.shape
        assert torch.equal(got.view(torch.int32)[mask], want.view(torch.int32)[mask]), "%s: stale packed weights (precision %d)" % (what, prec)
        assert model.packed(prec)[0] is got, "%s: re-packed although nothing changed" % what


def _render(scene, model):
    sahs = pkg()
    cfg, H = scene["cfg"], 8
    ro, rd = sahs.get_ray_bundle(H, H, scene["intr"], scene["pose"])
    cfg.nerf.validation.perturb = False
    with torch.no_grad():
        outs = sahs.run_one_iter_of_nerf(H, H, scene["intr"], model, ro, rd, cfg, mode="validation", driving=scene["drv"], pose=scene["pose"],
                                         background_prior=scene["bgp"].reshape(-1, 15)[:H * H].contiguous())
    return [o.clone() for o in outs if o is not None]


def _assert_renders_as_its_state_dict(scene, model, what):
    fresh = scene["model"]()
    fresh.load_state_dict({k: v.clone() for k, v in model.state_dict().items()})
    for a, b in zip(_render(scene, model), _render(scene, fresh)):
        assert torch.equal(a, b), "%s: the flattened model does not render what its state_dict renders" % what


# ---- 2. + 3. the step inside train_step, replayed; no stale weights ---------------------------------------------------------------------
@pytest.mark.parametrize("arch", ARCHS)
def test_train_step_with_flat_adam_replayed(arch):
    """Six train_steps with FlatAdam on a flattened model; the flat gradient and the learning rate captured before every update are
    replayed through torch.optim.Adam in fp32 and float64 on unflattened copies: the parameters must meet the yardstick of the update
    arithmetic (deterministic although the backward's atomics are not: the gradients are the captured ones).  After every step the
    packed streams (fp32 and bf16x3) are bit-identical to a pack of the buffer, and at the end -- and after load_flat, load_state_dict
    and an in-place edit of one parameter -- the model renders bit for bit what a fresh unflattened model with its state_dict renders."""
    Tr, ops = pkg("training"), pkg("ops")
    sc = _scene(arch)
    cfg = sc["cfg"]
    model = sc["model"]().flatten_parameters_()
    opt = Tr.FlatAdam(model, lr=cfg.optimizer.lr)
    caps = _capturing(opt, model)
    model.packed(ops.SAHS_BF16X3)                      # both precisions cached from the start
    g = torch.Generator(device=dev()).manual_seed(0)
    torch.manual_seed(0)
    sp = torch.ones(12, device=dev()) / 12
    for step in range(6):
        before = model.flat_params().clone()
        r = Tr.train_step(model, opt, cfg, step, *sc["args"], sp, generator=g)
        sp = r["sample_prob"]
        assert np.isfinite(r["loss"]) and not torch.equal(before, model.flat_params())
        _assert_fresh(model, "%s step %d" % (arch, step))
    assert len(caps) == 6 and all(bool(c[0].any()) and c[2] == 1.0 for c in caps)
    assert [c[1] for c in caps] == [cfg.optimizer.lr] + [Tr.learning_rate(cfg, s) for s in range(5)]
    for p in model.parameters():                       # the views survived six steps
        assert p.grad is not None
    model._check_flat_views()
    r32, r64 = _replay(sc, caps, cfg.optimizer.lr)
    assert np.abs(r32.astype(np.float64) - r64).max() > 0.0 and np.abs(r64 - sc["fw"]).max() > 0.0
    yardstick(model.flat_params(), r32, r64, "FlatAdam in train_step x6 (%s): params" % arch)
    _assert_renders_as_its_state_dict(sc, model, arch + " after 6 steps")
    # the other writers
    W = pkg("weights")
    model.load_flat(W.flatten_state_dict(W.hash_state_dict(1, 8.0, 30.0, model=arch), model=arch))
    _assert_fresh(model, arch + " load_flat")
    _assert_renders_as_its_state_dict(sc, model, arch + " after load_flat")
    model.load_state_dict({k: torch.from_numpy(v) for k, v in W.hash_state_dict(2, 8.0, 30.0, model=arch).items()})
    _assert_fresh(model, arch + " load_state_dict")
    _assert_renders_as_its_state_dict(sc, model, arch + " after load_state_dict")
    with torch.no_grad():
        model.nerf_mlps["fine"].fc_rgb.bias.add_(0.25)
    _assert_fresh(model, arch + " in-place edit")
    _assert_renders_as_its_state_dict(sc, model, arch + " after an in-place edit")


# ---- 4. training still trains -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("forward", ["fp32", "bf16x3"])
@pytest.mark.parametrize("arch", ARCHS)
def test_training_loop_with_flat_adam_reduces_loss(arch, forward):
    Tr, ops = pkg("training"), pkg("ops")
    sc = _scene(arch)
    cfg = sc["cfg"]
    model = sc["model"]().flatten_parameters_()
    opt = Tr.FlatAdam(model, lr=cfg.optimizer.lr)
    g = torch.Generator(device=dev()).manual_seed(0)
    torch.manual_seed(0)
    sp = torch.ones(12, device=dev()) / 12
    losses = []
    prev = ops.training_forward_precision()
    ops.training_forward_precision(forward)
    try:
        for step in range(8):
            r = Tr.train_step(model, opt, cfg, step, *sc["args"], sp, generator=g)
            sp = r["sample_prob"]
            losses.append(r["loss"])
            assert np.isfinite(r["loss"]) and abs(float(sp.sum()) - 1) < 1e-5
    finally:
        ops.training_forward_precision(prev)
    print(arch, forward, "losses", ["%.5f" % l for l in losses])
    assert min(losses[4:]) < losses[0], losses


# ---- 5. checkpoints interchange ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("writer", ["flat", "torch"])
def test_checkpoints_interchange(writer, tmp_path):
    """Three train_steps with one optimiser class, save_checkpoint, resume into the other class (and into torch.optim.Adam in float64);
    one further update with the same injected gradient leaves all of them with the same parameters under the update's yardstick."""
    Tr = pkg("training")
    arch = "nerface_static"
    sc = _scene(arch, rays=256)
    cfg = sc["cfg"]

    def make(flat, dtype=torch.float32):
        m = sc["model"]()
        if dtype == torch.float64:
            m = m.double()
        if flat:
            return m.flatten_parameters_(), Tr.FlatAdam(m, lr=cfg.optimizer.lr)
        return m, torch.optim.Adam(m.parameters(), lr=cfg.optimizer.lr, foreach=False)

    model, opt = make(writer == "flat")
    g = torch.Generator(device=dev()).manual_seed(0)
    sp = torch.ones(12, device=dev()) / 12
    for step in range(3):
        sp = Tr.train_step(model, opt, cfg, step, *sc["args"], sp, generator=g)["sample_prob"]
    path = str(tmp_path / "ck.pt")
    Tr.save_checkpoint(path, 3, model, opt, 0.0, sample_prob=sp)
    n = sum(p.numel() for p in model.parameters())
    inject = torch.randn(n, device=dev(), generator=torch.Generator(device=dev()).manual_seed(77)) * 1e-2
    flats = {}
    for name, (flat, dtype) in dict(flat=(True, torch.float32), torch=(False, torch.float32), f64=(False, torch.float64)).items():
        m, o = make(flat, dtype)
        info = Tr.resume(path, m, o, dev())
        assert info["start_iter"] == 4 and torch.equal(info["sample_prob"], sp)
        for k, v in model.state_dict().items():
            assert torch.equal(m.state_dict()[k].float(), v), k
        sd = o.state_dict()
        assert len(sd["state"]) == len(list(m.parameters())) and float(sd["state"][0]["step"]) == 3.0
        off = 0
        for p in m.parameters():
            gp = inject[off:off + p.numel()].to(dtype).view_as(p)
            if p.grad is None:
                p.grad = gp.clone()
            else:
                p.grad.copy_(gp)
            off += p.numel()
        o.step()
        assert float(o.state_dict()["state"][0]["step"]) == 4.0
        flats[name] = torch.cat([p.detach().reshape(-1) for p in m.parameters()]).cpu().numpy()
    assert np.abs(flats["torch"].astype(np.float64) - flats["f64"]).max() > 0.0
    yardstick(flats["flat"], flats["torch"], flats["f64"], "checkpoint written by %s Adam, one more update: params" % writer)


# ---- 6. data parallel -------------------------------------------------------------------------------------------------------------------
def _dp_worker(rank, world, port, path):
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        Tr = pkg("training")
        sc = _scene("audio", rays=256)
        cfg = sc["cfg"]
        model = sc["model"]().flatten_parameters_()
        opt = Tr.FlatAdam(model, lr=float(cfg.optimizer.lr))
        caps = _capturing(opt, model)
        prob = torch.ones(12, device=dev()) / 12
        torch.manual_seed(100 + rank)          # the ranks' own noise streams differ; the batch draw does not
        for step in range(2):
            out = Tr.train_step(model, opt, cfg, step, *sc["args"], prob, generator=torch.Generator(device=dev()).manual_seed(9 + step))
            prob = out["sample_prob"]
        assert [c[2] for c in caps] == [0.5, 0.5]       # the kernel averages as it reads: 1 / world
        flat = model.flat_params().cpu()
        both = [torch.zeros_like(flat) for _ in range(world)]
        dist.all_gather(both, flat)
        assert torch.equal(both[0], both[1]), "the replicas diverged: max %.3e" % float((both[0] - both[1]).abs().max())
        grads = [c[0].cpu() for c in caps]
        for gk in grads:                                # the captured gradients are the REDUCED ones: the same on both ranks
            pair = [torch.zeros_like(gk) for _ in range(world)]
            dist.all_gather(pair, gk)
            assert torch.equal(pair[0], pair[1]) and bool(gk.any())
        model._check_flat_views()
        if rank == 0:
            r32, r64 = _replay(sc, caps, float(cfg.optimizer.lr))
            assert np.abs(r32.astype(np.float64) - r64).max() > 0.0
            yardstick(flat, r32, r64, "FlatAdam, two data-parallel ranks x2 steps: params")
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_two_ranks_train_data_parallel_with_flat_adam(tmp_path):
    """training.train_step with FlatAdam on two ranks (both on the one GPU, gloo): the flat gradient buffer is all-reduced in place and
    scaled by 1 / world inside the optimiser kernel; after two steps the replicas' flat buffers are bit-identical and meet the update's
    yardstick against a replay of the reduced gradients, times 1 / world, through torch.optim.Adam in fp32 and float64."""
    _run_ranks(free_port(), str(tmp_path))


def _run_ranks(port, path, limit=420):
    ctx = mp.start_processes(_dp_worker, args=(2, port, path), nprocs=2, join=False, start_method="spawn")
    t0 = time.time()
    try:
        while not ctx.join(timeout=5):
            if time.time() - t0 > limit:
                raise TimeoutError("the two ranks did not finish within %d s" % limit)
    finally:
        for p in ctx.processes:
            if p.is_alive():
                p.kill()
