"""Training step of the dual-stream denoiser on the MI355X (SURVEY section 8a device op 11, cfg 4; reference
train/train.py:1258-1427): the reference's x0-prediction losses over the differentiable forward of ``autograd_net``
(AttributeEncoderModel -> UNet2DConditionModel -> AttributeDecoderModel), the backward, the data-parallel gradient
all-reduce of ``parallel.GradientBuckets`` (RCCL over xGMI, one flat bucket list for the three networks instead of the
reference's three DDP wrappers, train.py:1140-1142), clipping folded into the optimizer pass, the update and the EMA step;
``GraphedTrainStep`` is the same step as HIP-graph replays.  The network forwards are re-exported for their importers here.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import torch

from . import backward as B
from .autograd_net import (FREEU_AUTOGRAD_MSG, LORA_AUTOGRAD_MSG, controlnet_forward, decoder_forward,  # noqa: F401
                           dual_stream_forward, encoder_forward, to_nhwc_grad, unet_forward)


def mse_losses(out: Dict[str, torch.Tensor], target_img: torch.Tensor, target_attr: Optional[torch.Tensor]) -> torch.Tensor:
    """The x0-prediction losses of train.py:1356-1365: mean squared error of both predictions against the clean
    latents (targets NCHW fp32)."""
    loss = torch.mean((out["img_pred"].float() - target_img.permute(0, 2, 3, 1).float()) ** 2)
    if "attr_pred" in out and target_attr is not None:
        loss = loss + torch.mean((out["attr_pred"].float() - target_attr.permute(0, 2, 3, 1).float()) ** 2)
    return loss


def reference_losses(nets: Sequence[torch.nn.Module], batch: Dict[str, torch.Tensor], dtype=torch.bfloat16,
                     inverse: bool = True) -> Dict[str, torch.Tensor]:
    """The losses of train/train.py:1356-1413 on one micro-batch.

    batch: ``x_t`` [B,4,h,w] noisy image latent, ``cond`` [B,28,h,w] = clean mask latent (4) | noisy attribute latents
    (24), ``ehs``, ``t_img``, ``t_attr``, ``target_img`` [B,4,h,w], ``target_attr`` [B,24,h,w]; for the inverse-rendering
    branch also ``x_t_c`` / ``t_img_c`` (a fresh noising of the image latent).

    loss = mse(img) + 10 mse(attr) + 0.01 contrastive (albedo of samples 0 / 1 positive; material, specular negative), or
    -- inverse rendering -- mse(img) + mse(attr) + 0.8 mse(img_c), where img_c is the UNet's prediction when the encoder
    is conditioned on [mask | the decoder's OWN attribute prediction] at t_attr = 0 (gradient flows through it)."""
    unet, enc, dec = nets
    F = torch.nn.functional
    out = dual_stream_forward(unet, enc, dec, batch["x_t"], batch["cond"], batch["ehs"], batch["t_img"], batch["t_attr"],
                              dtype=dtype)
    nhwc = lambda t: t.permute(0, 2, 3, 1).float()
    mask_pred = out["attr_pred"][..., 4:]  # rule out the clean mask group (train.py:1354)
    loss_img = F.mse_loss(out["img_pred"].float(), nhwc(batch["target_img"]))
    loss_mask = F.mse_loss(mask_pred.float(), nhwc(batch["target_attr"]))
    res = {"loss_img": loss_img, "loss_mask": loss_mask}
    if not inverse:
        cos = lambda a: F.cosine_similarity(a[0].reshape(-1).float(), a[1].reshape(-1).float(), dim=0) / 0.1
        m_dis, a_dis, s_dis = cos(mask_pred[..., :4]), cos(mask_pred[..., 8:12]), cos(mask_pred[..., 12:16])
        pos = torch.exp(a_dis)
        res["contrastive"] = -torch.log(pos / (pos + torch.exp(m_dis) + torch.exp(s_dis)))
        res["loss"] = loss_img + loss_mask * 10.0 + res["contrastive"] * 0.01
        return res
    mask_lat = batch["cond"][:, :4].permute(0, 2, 3, 1).to(dtype)
    cond_c = torch.cat((mask_lat, mask_pred), dim=-1)
    B = batch["x_t"].shape[0]
    out_c = dual_stream_forward(unet, enc, dec, batch["x_t_c"], None, batch["ehs"], batch["t_img_c"],
                                torch.zeros(B, device=batch["x_t"].device), dtype=dtype, run_decoder=False, cond_nhwc=cond_c)
    res["loss_c"] = F.mse_loss(out_c["img_pred"].float(), nhwc(batch["target_img"]))
    res["loss"] = loss_img + loss_mask + 0.8 * res["loss_c"]
    return res


def _forward_backward(nets, batch, optimizer, buckets, dtype, inverse, grad_accum=None, loss_scale=None, scaler=None):
    """forward, losses, backward; gradients end in ``buckets``' flat buffers (collectives of complete buckets already in
    flight when the buckets were built with ``overlap=True``) or in fresh ``p.grad`` tensors.
    ``grad_accum`` = (k, n): micro-step k of n of one optimisation step (train.py:1236 ``accelerator.accumulate``):
    gradients are zeroed only at k = 0, the loss is divided by n (accelerate's ``backward``), and with ``buckets`` every
    micro-step but the last runs under ``no_sync()``.  ``loss_scale``: a factor (device scalar or float) the loss is
    multiplied with before ``backward()``; ``scaler``: a ``torch.amp.GradScaler`` whose ``scale(loss)`` is used instead
    (train.sh:21 ``--mixed_precision="fp16"``: accelerate's ``backward`` does exactly that)."""
    unet, enc, dec = nets
    k, n = grad_accum if grad_accum is not None else (0, 1)
    if inverse is None:
        out = dual_stream_forward(unet, enc, dec, batch["x_t"], batch["cond"], batch["ehs"], batch["t_img"],
                                  batch["t_attr"], dtype=dtype)
        loss = mse_losses(out, batch["target_img"], batch["target_attr"])
    else:
        loss = reference_losses(nets, batch, dtype=dtype, inverse=inverse)["loss"]
    if k == 0:
        if buckets is not None:
            buckets.zero_grad()  # gradients live in the buckets' flat buffers (views): zero in place, keep the views
        elif optimizer is not None:
            optimizer.zero_grad(set_to_none=True)
    # per-launch sums of squares of the fp32 gradients written by this backward (clipping norm).  They describe the
    # gradients only if this backward produces them from scratch: one micro-step, no loss scaling, and no parameter of
    # these networks holding an older gradient (an optimizer over a subset of the parameters zeroes only its own)
    fresh = (n == 1 and loss_scale is None and scaler is None and buckets is None
             and all(p.grad is None for p in _parameters(nets)))
    B.grad_squares.begin(token=_nets_token(nets), trusted=fresh)
    B.wgrad_queue.reset()
    report = loss.detach()
    if n > 1:
        loss = loss / n
    if loss_scale is not None:
        loss = loss * loss_scale
    if scaler is not None:
        loss = scaler.scale(loss)
    if buckets is not None and k + 1 < n:
        with buckets.no_sync():
            loss.backward()
    else:
        loss.backward()  # with ``buckets``: complete buckets are all-reduced (async) while the backward is still running
    B.wgrad_queue.flush()  # nothing pending after a complete backward (CastParams / ParamBarrier flush); a partial graph may leave some
    if buckets is not None and getattr(buckets, "direct_write", False) and not buckets._hooks:
        # no hooks adopted stray gradients during the backward (overlap=False / gloo): do it here, inside a capture if there is one
        buckets.adopt_all()
    return report


_param_cache: Dict[tuple, tuple] = {}


def _nets_token(nets) -> tuple:
    return tuple(id(n) for n in nets)


def _parameters(nets) -> list:
    """All parameters of the networks, cached per network triple: walking ``Module.parameters()`` of ~700 tensors costs
    ~7 ms of host time, at the tail of a host-bound eager step every time it is done."""
    key = tuple(id(n) for n in nets)
    hit = _param_cache.get(key)
    if hit is None or any(a is not b for a, b in zip(hit[0], nets)):  # (the networks themselves, their parameters)
        hit = _param_cache[key] = (tuple(nets), [p for n in nets for p in n.parameters()])
    return hit[1]


def _ema_list(nets, ema) -> list:
    """``ema`` of train_step / GraphedTrainStep as [(EMAModel, the parameters it averages)]: one ``training_utils.EMAModel`` over
    all parameters of ``nets`` in order, or a sequence with one entry (or None) per network, as the diffusers scripts keep one
    ``ema_unet`` per model."""
    if ema is None:
        return []
    if hasattr(ema, "shadow_params"):
        return [(ema, _parameters(nets))]
    ema = list(ema)
    if len(ema) != len(nets):
        raise ValueError(f"ema: {len(ema)} EMAModels for {len(nets)} networks (pass one per network, None to leave one out)")
    return [(e, _parameters((n,))) for e, n in zip(ema, nets) if e is not None]


def _clip_and_update(nets, optimizer, buckets, max_grad_norm, stats, scaler=None, ema=None):
    """train.py:1422-1425: clip_grad_norm_ + optimizer.step(), the clipping folded into the optimizer pass when it can.
    With ``scaler`` (fp16 AMP, train.sh:21): the reference's order -- ``unscale_`` (which also looks for inf / nan),
    clip, ``scaler.step`` (skips the update when an overflow was found: parameters, moments and the step counter stay),
    ``scaler.update``.  ``ema``: the averages step after the update (also after one the scaler skipped, as in the diffusers
    scripts)."""
    _update(nets, optimizer, buckets, max_grad_norm, stats, scaler)
    for e, params in _ema_list(nets, ema):
        e.step(params)


def _update(nets, optimizer, buckets, max_grad_norm, stats, scaler):
    if scaler is not None:
        if optimizer is None:
            raise ValueError("a GradScaler needs the optimizer whose gradients it unscales")
        scaler.unscale_(optimizer)
        if max_grad_norm is not None:
            if buckets is not None:
                stats["grad_norm"] = buckets.clip_grad_norm_(max_grad_norm)
            else:
                params = [p for p in _parameters(nets) if p.grad is not None]
                stats["grad_norm"] = torch.nn.utils.clip_grad_norm_(params, max_grad_norm)
        scaler.step(optimizer)
        scaler.update()
        return
    folded = False
    if max_grad_norm is not None:
        # torch's fused Adam / AdamW kernels (and optim.FusedAdamW) divide every gradient by ``optimizer.grad_scale`` on
        # the fly (the hook GradScaler uses): handing them 1 / clip_coefficient applies train.py:1422-1424's clipping
        # inside the optimizer pass instead of a separate read-modify-write sweep over 7 GB of gradients
        fold = (optimizer is not None and getattr(optimizer, "_step_supports_amp_scaling", False)
                and all(g.get("fused") for g in optimizer.param_groups))
        if fold:
            if buckets is not None and getattr(buckets, "sumsq_parts", None):
                # finish() converted the reduced half-precision buckets back to fp32 and summed the squares in the same pass
                norm = torch.cat(buckets.sumsq_parts).sum().sqrt()
                buckets.sumsq_parts = None
            elif buckets is not None:
                # _foreach_norm, not vector_norm per bucket: a CAPTURED vector_norm over a 32 MB tensor returns wrong
                # values on replay in this torch / ROCm build (tools/graph_norm_repro.py)
                norm = torch.linalg.vector_norm(torch.stack(torch._foreach_norm(list(buckets.flat))))
            elif B.FUSED_GRADNORM and B.grad_squares.usable(_nets_token(nets)):
                # the big gradients' sums of squares came out of the kernels that wrote them; only the parameters those
                # launches do not cover (norm / bias vectors, a few small matrices) are swept here
                cov = B.grad_squares.count
                rest = [p.grad for p in _parameters(nets) if p.grad is not None and id(p) not in cov]
                sq = torch.cat(B.grad_squares.parts).sum()
                if rest:
                    sq = sq + torch.stack(torch._foreach_norm(rest)).square().sum()
                norm = sq.sqrt()
                B.grad_squares.clear()  # consumed: stale partial sums must not describe a later step
            else:
                grads = [p.grad for p in _parameters(nets) if p.grad is not None]
                norm = torch.linalg.vector_norm(torch.stack(torch._foreach_norm(grads)))
            stats["grad_norm"] = norm
            optimizer.grad_scale = torch.clamp((norm + 1e-6) / max_grad_norm, min=1.0).to(torch.float32).reshape(())
            optimizer.found_inf = torch.zeros((), dtype=torch.float32, device=norm.device)
            folded = True
        elif buckets is not None:
            stats["grad_norm"] = buckets.clip_grad_norm_(max_grad_norm)
        else:
            params = [p for p in _parameters(nets) if p.grad is not None]
            stats["grad_norm"] = torch.nn.utils.clip_grad_norm_(params, max_grad_norm)
    if optimizer is not None:
        optimizer.step()
        if folded:
            del optimizer.grad_scale, optimizer.found_inf


def train_step(nets: Sequence[torch.nn.Module], batch: Dict[str, torch.Tensor], optimizer=None, buckets=None,
               dtype=torch.bfloat16, max_grad_norm: Optional[float] = 1.0, inverse: Optional[bool] = None,
               as_tensors: bool = False, grad_accum: Optional[tuple] = None, scaler=None, ema=None) -> Dict[str, float]:
    """One optimisation step: forward, losses, backward (HIP kernels), gradient all-reduce (``buckets``: a
    parallel.GradientBuckets, no-op on one rank), clipping (train.py:1422-1424), optimizer step.
    ``grad_accum`` = (k, n): micro-step k of n (``accelerator.accumulate``, train.py:1236): gradients are zeroed at
    k = 0 only, the loss is divided by n, the collectives / clipping / update happen at k = n - 1 only.
    ``scaler``: a ``torch.amp.GradScaler`` for the reference's fp16 AMP recipe (train.sh:21; pass ``dtype=torch.float16``).
    ``inverse``: None = the plain two-stream MSE objective (mse_losses); True / False = the reference's inverse-rendering
    (cycle consistency) / rendering (contrastive) objectives (reference_losses).  Ranks may pick different branches
    (compute_t, train.py:445): parameters without a gradient contribute zeros to the buckets.
    ``as_tensors``: return the statistics as device tensors (no host synchronisation: the step can then be captured
    into a HIP graph, tools/train_bench.py --graph).
    ``ema``: a ``training_utils.EMAModel`` over all parameters of ``nets``, or a sequence of them, one per network (None to
    leave one out): each takes its ``step()`` after the optimizer update (diffusers' ``--use_ema``)."""
    if ema is not None and optimizer is None:
        raise ValueError("ema needs the optimizer whose update it follows")
    _ema_list(nets, ema)  # a wrong count raises before anything ran
    stats = {"loss": _forward_backward(nets, batch, optimizer, buckets, dtype, inverse, grad_accum=grad_accum, scaler=scaler)}
    last = grad_accum is None or grad_accum[0] + 1 == grad_accum[1]
    if buckets is not None:
        if last:
            buckets.finish()
        else:
            with buckets.no_sync():
                buckets.finish()  # an accumulation micro-step: only adopts gradients re-created outside the buckets
    if last:
        _clip_and_update(nets, optimizer, buckets, max_grad_norm, stats, scaler=scaler, ema=ema)
    return stats if as_tensors else {k: float(v) for k, v in stats.items()}


class GraphedTrainStep:
    """The training step as HIP-graph replays, also on several GPUs.

    Eagerly the step is host-bound (~9700 launches issued from Python: 118 ms against 90 ms of GPU work at cfg 4's
    per-GPU shape), which is also what bounds the data-parallel step when the gradient collectives are launched from
    autograd hooks.  Here forward + losses + backward are ONE captured graph writing the gradients into the flat bucket
    buffers of ``buckets`` (built with ``overlap=False``: no hooks, nothing but kernels inside the capture); the
    collectives run eagerly on those few flat buffers (``buckets.finish()``: one all-reduce or reduce-scatter +
    all-gather per 256 MB bucket, bf16 on the wire if asked), and clipping + the optimizer step are a second graph.
    Without ``buckets`` (one GPU) the whole step is a single graph.  One instance per objective branch (``inverse``):
    the branch is a host decision (train.py:445), so a training loop keeps one instance per branch over the same
    networks and optimizer.  ``warmup`` eager steps run first (REAL optimisation steps on ``batch``: allocator pools, lazy
    optimizer state); 0 is allowed with optimizers whose state can be created up front (optim.FusedAdamW).
    The optimizer's lr / betas / eps / weight_decay are captured by value; ``step()`` notices when a scheduler or a resumed
    checkpoint changed them and captures again."""

    def __init__(self, nets, batch: Dict[str, torch.Tensor], optimizer, buckets=None, dtype=torch.bfloat16,
                 max_grad_norm: Optional[float] = 1.0, inverse: Optional[bool] = None, warmup: int = 2,
                 capture_collectives: Optional[bool] = None, ema=None):
        """``ema``: as in ``train_step``.  The averages step in the warm-up steps (they are real optimisation steps) and INSIDE
        the captured graph, behind the optimizer update (without buckets the one graph, with them the update graph): their
        decay schedule lives in device memory, so every replay advances it by itself.

        ``capture_collectives`` (RCCL only; default: on when ``buckets`` were built with ``overlap=True`` on the nccl
        backend): the bucket collectives are captured INTO the step graph.  The post-accumulate hooks of ``buckets`` enqueue
        each bucket's all-reduce / reduce-scatter + all-gather on RCCL's stream the moment the bucket is complete -- inside a
        capture that is a fork: the collective becomes a parallel branch of the graph that runs beside the rest of the
        backward, joined by ``buckets.finish()`` in front of clipping + update.  With the weight gradients deferred to the end
        of each network's backward (backward.WgradQueue) the buckets complete network by network: the decoder's collectives
        overlap the UNet's backward, the UNet's the encoder's -- DDP's overlap at train/train.py:1421, with the whole step
        ONE replay and no host in the loop.  Without it (gloo, or ``overlap=False`` buckets): forward + backward graph,
        eager collectives, update graph, serially."""
        import torch.distributed as dist
        hooks = bool(buckets is not None and getattr(buckets, "_hooks", None))
        nccl = bool(buckets is not None and dist.is_initialized() and dist.get_backend(getattr(buckets, "group", None)) == "nccl")
        if capture_collectives is None:
            capture_collectives = hooks and nccl
        if capture_collectives and not (hooks and nccl):
            raise ValueError("capture_collectives needs GradientBuckets(..., overlap=True) on the nccl (RCCL) backend")
        if hooks and not capture_collectives:
            raise ValueError("GraphedTrainStep without captured collectives needs GradientBuckets(..., overlap=False): "
                             "hooks launching eager collectives cannot run inside a capture")
        self.capture_collectives = bool(capture_collectives)
        if self.capture_collectives:  # RCCL creates its communicator on first use: that must not happen inside a capture
            t = torch.zeros(8, device=buckets.flat[0].device)
            dist.all_reduce(t, group=buckets.group)
            torch.cuda.synchronize()
        self.nets, self.optimizer, self.buckets, self.ema = nets, optimizer, buckets, ema
        _ema_list(nets, ema)  # a wrong count raises before anything ran
        # gloo (the CPU-side test transport) stages device tensors through the host; handing it a tensor whose producer
        # graph is still replaying was measured at 50-140 s per step with two ranks on one GPU (0.03 s after a stream
        # synchronise).  RCCL collectives are stream-ordered and need no host wait.
        self._host_sync_before_collectives = bool(buckets is not None and dist.is_initialized()
                                                  and dist.get_backend(getattr(buckets, "group", None)) == "gloo")
        self.batch = {k: v.clone() for k, v in batch.items()}
        self.stats: Dict[str, torch.Tensor] = {}
        kw = dict(dtype=dtype, inverse=inverse)
        if warmup == 0:
            # nothing may be created lazily inside the capture (a zero-fill captured there would re-run on every replay)
            init = getattr(optimizer, "_init_state", None)
            if init is None:
                raise ValueError("warmup=0 needs an optimizer that can create its state eagerly (optim.FusedAdamW)")
            for grp in optimizer.param_groups:
                for p in grp["params"]:
                    if p.requires_grad:
                        init(p)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(warmup):  # allocator pools, lazy optimizer state, the tuning-table lookups
                self._eager(kw, max_grad_norm)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        self.max_grad_norm = max_grad_norm
        self._kw = kw
        self._updated = [p for grp in optimizer.param_groups for p in grp["params"] if p.requires_grad]
        self._updated += [s for e, _ in _ema_list(nets, ema) for s in e.shadow_params]  # written by the captured step too
        self._capture()

    def _hyper(self):
        """The optimizer hyper-parameters the captured update holds BY VALUE (kernel arguments of ``ur_adamw_multi``).
        lr and weight_decay are NOT among them when the optimizer keeps them in device memory (optim.FusedAdamW.sync_hyper):
        a scheduler step then only needs that copy refreshed before the replay."""
        dev_lr = hasattr(self.optimizer, "sync_hyper")
        # ... and the ADDRESSES it holds: the device (lr, weight_decay) pair and the optimizer's ``generation`` (bumped when
        # load_state_dict / add_param_group replaced state tensors a captured update points at)
        return (getattr(self.optimizer, "generation", 0),) + tuple(e.generation for e, _ in _ema_list(self.nets, self.ema)) + tuple(
            ((None if dev_lr else float(g["lr"])), tuple(float(b) for b in g["betas"]), float(g["eps"]),
             (None if dev_lr else float(g["weight_decay"])),
             (g["_ur_hyper"][0].data_ptr() if g.get("_ur_hyper") is not None else None)) for g in self.optimizer.param_groups)

    def _capture(self):
        nets, optimizer, buckets, kw, max_grad_norm = self.nets, self.optimizer, self.buckets, self._kw, self.max_grad_norm
        if hasattr(optimizer, "sync_hyper"):
            optimizer.sync_hyper()
        self._captured_hyper = self._hyper()
        self.g_fb = torch.cuda.CUDAGraph()
        self.g_up = None
        if self.capture_collectives:
            buckets._reset()
            if buckets.fused_sumsq():
                buckets.sumsq_buffers()  # allocated outside the capture: finish() writes them inside it and in eager steps
            before = buckets.launched_from_hooks
            with torch.cuda.graph(self.g_fb):
                # the hooks fire inside backward(): every complete bucket's collective forks onto RCCL's stream here
                self.stats["loss"] = _forward_backward(nets, self.batch, None, buckets, **kw)
                self.collectives_from_hooks = buckets.launched_from_hooks - before  # forked before finish() had to
                buckets.finish()  # launches what the hooks could not, then joins RCCL's stream (work.wait = stream wait)
                _clip_and_update(nets, optimizer, buckets, max_grad_norm, self.stats, ema=self.ema)
            self._validate_captured_collectives()
            return
        with torch.cuda.graph(self.g_fb):
            self.stats["loss"] = _forward_backward(nets, self.batch, optimizer if buckets is None else None, buckets, **kw)
            if buckets is None:
                _clip_and_update(nets, optimizer, None, max_grad_norm, self.stats, ema=self.ema)
        if buckets is not None:
            buckets._reset()
            # the eager finish() before every replay leaves the clipping norm's sums of squares in fixed buffers when the
            # transport is half precision: capture the update reading them, the norm the eager step uses (a captured
            # _foreach_norm over the buckets sums in another order, and the clip coefficient would differ in the last bits)
            buckets.sumsq_parts = buckets.sumsq_buffers() if buckets.fused_sumsq() else None
            self.g_up = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.g_up):
                _clip_and_update(nets, optimizer, buckets, max_grad_norm, self.stats, ema=self.ema)
            buckets.sumsq_parts = None

    def _validate_captured_collectives(self):
        """The split "forked by a hook during the backward" / "launched by finish()" is baked into the graph at capture time.
        Buckets always launch in index order (GradientBuckets._launch), so the SEQUENCE of collectives is the same on every
        rank by construction; what could differ is where they sit in each rank's graph -- harmless for correctness (RCCL
        matches them by order on its own stream), but a rank whose buckets all fell to finish() serialises every other rank's
        overlap behind its backward.  Cross-check the count once per capture and refuse a mixed capture: a
        parameter that got no gradient on one rank during the capture step would otherwise go unnoticed for the whole run."""
        import torch.distributed as dist
        b = self.buckets
        if not dist.is_initialized() or dist.get_world_size(b.group) < 2:
            return
        n = float(self.collectives_from_hooks)
        t = torch.tensor([n, -n], dtype=torch.float32, device=b.flat[0].device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX, group=b.group)
        hi, lo = float(t[0]), -float(t[1])
        if hi != lo:
            raise RuntimeError(f"captured bucket collectives differ across ranks: between {int(lo)} and {int(hi)} of {len(b.buckets)} "
                               "buckets were launched from the backward's hooks (a parameter without a gradient on some rank "
                               "during the capture step?); capture with a batch that reaches every parameter on every rank")

    def _ensure_current(self):
        """Refresh the device (lr, weight_decay) pair and capture again if a hyper-parameter held by value, or an address the
        captured update points at, changed since the capture."""
        if hasattr(self.optimizer, "sync_hyper"):
            self.optimizer.sync_hyper()  # lr / weight_decay of an lr_scheduler step -> the device pair the kernel reads
        if self._hyper() != self._captured_hyper:
            # betas / eps changed (resume_from_checkpoint with other settings), or an optimizer that holds lr by value:
            # the captured update has the old values as kernel arguments.  Capture again (tens of ms, once per change)
            torch.cuda.synchronize()
            self._capture()

    def _eager(self, kw, max_grad_norm):
        st = {"loss": _forward_backward(self.nets, self.batch, self.optimizer, self.buckets, **kw)}
        if self.buckets is not None:
            self.buckets.finish()
        _clip_and_update(self.nets, self.optimizer, self.buckets, max_grad_norm, st, ema=self.ema)

    def step(self, batch: Optional[Dict[str, torch.Tensor]] = None) -> Dict[str, torch.Tensor]:
        """One optimisation step on ``batch`` (copied into the captured input buffers; None: the last one again).
        Returns device tensors (loss, grad_norm): reading them is the caller's synchronisation."""
        if batch is not None:
            for k, v in batch.items():
                self.batch[k].copy_(v)
        self._ensure_current()
        self.g_fb.replay()
        if self.buckets is not None and not self.capture_collectives:
            if self._host_sync_before_collectives:
                torch.cuda.current_stream().synchronize()
            self.buckets.finish()
            self.g_up.replay()  # clipping (torch._foreach_norm over the buckets) + optimizer step
        # a replay runs no Python: bump the version counters of what the captured update wrote, as the eager optimizer step does,
        # so that packed copies, inference graphs and a merged LoRA adapter notice the new values
        torch.autograd.graph.increment_version(self._updated)
        return self.stats

    def phase_times(self) -> Dict[str, float]:
        """One step with HIP events between the phases (synchronises): milliseconds of the forward + backward replay, of the
        bucket collectives (launch to completion, as the compute stream sees them) and of clipping + update.  With captured
        collectives the step is one graph and only its total is observable from outside (``overlapped_total``)."""
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        self._ensure_current()  # the same staleness check as step(): never replay an update holding freed addresses
        ev[0].record()
        self.g_fb.replay()
        ev[1].record()
        if self.buckets is not None and not self.capture_collectives:
            if self._host_sync_before_collectives:
                torch.cuda.current_stream().synchronize()
            self.buckets.finish()
            ev[2].record()
            self.g_up.replay()
        else:
            ev[2].record()
        ev[3].record()
        torch.cuda.synchronize()
        if self.capture_collectives or self.buckets is None:
            return dict(overlapped_total=ev[0].elapsed_time(ev[3]))
        return dict(replay=ev[0].elapsed_time(ev[1]), collectives=ev[1].elapsed_time(ev[2]), update=ev[2].elapsed_time(ev[3]))
