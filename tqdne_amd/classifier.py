"""Classifier (second stage of the reference's workflow; drop-in for ``tqdne.classifier.LithningClassifier``, classifier.py:9-92):
the ``Encoder`` trunk, mean over time, ``output_MLP`` and ``output_layer``.  Same constructor, attributes and ``state_dict`` schema
(``encoder.*``, ``output_MLP.1.*``, ``output_MLP.3.*``, ``output_layer.*`` and the loss module's own entries, e.g. ``loss.weight``).

dims=1: the encoder plan runs on the HIP kernels and ends channels-last (B, T', C); the head reads it there (no NCW copy):
``tq_classifier_head_fwd`` forward, ``tq_classifier_head_bwd`` backward -- which writes d loss / d h straight into the channels-last
gradient buffer of the encoder's backward plan -- and ``tq_cross_entropy`` for the loss of the training route (csrc/classifier.hip).
dims=2: the encoder goes through family2d (stock PyTorch) and the head is the same torch modules under autograd.
"""

from __future__ import annotations

import torch as th
from torch import nn

from . import engine, rng
from .autoencoder import Encoder, _seq_engine
from .autograd import check_fresh
from .lightning_compat import HAVE_LIGHTNING, LightningModule

try:  # pragma: no cover - not installed in the build image
    from torchmetrics import MetricCollection
except Exception:  # ImportError and friends
    class MetricCollection(nn.Module):
        """Stand-in where torchmetrics is not installed: calls every metric with (preds, target) and returns {name: value}.
        Metrics that are modules are registered (they follow ``.to()``); it owns no arithmetic and no ``state_dict`` entry of its own."""

        def __init__(self, metrics=()):
            super().__init__()
            items = list(metrics.items()) if isinstance(metrics, dict) else [(type(m).__name__, m) for m in metrics]
            self._names = [n for n, _ in items]
            self._plain = {}
            for n, m in items:
                if isinstance(m, nn.Module):
                    self.add_module(n, m)
                else:
                    self._plain[n] = m

        def _metric(self, n):
            return self._plain[n] if n in self._plain else getattr(self, n)

        def forward(self, preds, target):
            return {n: self._metric(n)(preds, target) for n in self._names}

        def __len__(self):
            return len(self._names)


def _head_limits():
    from . import _lib
    lib = _lib.load()
    return lib.tq_classifier_head_max_channels(), lib.tq_classifier_head_max_classes()


class _HeadFn(th.autograd.Function):
    """``embed`` / ``forward`` of the 1-D classifier as an ordinary differentiable call: the HIP forward keeps what a backward reads
    (the encoder plan's activations, pooled / a1 / emb of the head); ``backward`` runs the HIP head backward seeded with the incoming
    gradient and then the encoder's sweep from the channels-last gradient the head wrote.  Gradients: every parameter, and the input
    when it requires one."""

    @staticmethod
    def forward(ctx, module, x, want_logits, *params):
        train = module.training
        out, eng, bufs = module._head_forward(x, want_logits, train, rng.next_dropout_seed() if train else 0)
        if eng.check_range():   # activations near the fp16 range: the plan is on bf16x3 now, repeat
            out, eng, bufs = module._head_forward(x, want_logits, train, rng.next_dropout_seed() if train else 0)
        ctx.module, ctx.eng, ctx.bufs, ctx.fwd_id = module, eng, bufs, eng._fwd_count
        ctx.want_logits, ctx.want_dx = want_logits, bool(x.requires_grad)
        return out.clone()

    @staticmethod
    def backward(ctx, gout):
        eng = ctx.eng
        check_fresh(eng, ctx.fwd_id)
        with th.no_grad():
            head = ctx.module._head_backward(eng, ctx.bufs, gout.contiguous().float(), ctx.want_logits)
            g_enc, dx = eng.backward(None, want_dx=ctx.want_dx, clone=True)
        return (None, dx, None) + tuple(g_enc) + tuple(head)


class LithningClassifier(LightningModule):
    """classifier.py:9-92.  ``encoder_config``: keywords of ``Encoder``; on the HIP path (dims=1) ``out_channels`` must be a multiple of
    32 up to ``tq_classifier_head_max_channels()`` and ``num_classes`` at most ``tq_classifier_head_max_classes()``."""

    def __init__(self, encoder_config: dict, num_classes: int, loss: nn.Module, metrics: list, optimizer_params: dict):
        super().__init__()
        out_channels = encoder_config["out_channels"]
        if encoder_config.get("dims", 2) == 1:
            max_c, max_k = _head_limits()
            if out_channels % 32 or not 32 <= out_channels <= max_c:
                raise NotImplementedError(
                    f"classifier: encoder out_channels = {out_channels}: the HIP head reads the channels-last output of the generic conv, "
                    f"which needs a multiple of 32 channels, up to {max_c} (tq_classifier_head_max_channels)")
            if not 1 <= num_classes <= max_k:
                raise NotImplementedError(f"classifier: num_classes = {num_classes}: the HIP head takes up to {max_k} classes "
                                          "(tq_classifier_head_max_classes)")
        self.encoder = Encoder(**encoder_config)
        self.output_MLP = nn.Sequential(nn.SiLU(), nn.Linear(out_channels, out_channels), nn.SiLU(),
                                        nn.Linear(out_channels, out_channels))
        self.output_layer = nn.Linear(out_channels, num_classes)
        self.loss = loss
        self.metrics = MetricCollection(metrics)
        self.optimizer_params = optimizer_params
        self.save_hyperparameters()

    def _apply(self, fn, *a, **k):
        self.__dict__.pop("_head_bufs", None)
        return super()._apply(fn, *a, **k)

    # ------------------------------------------------------------------ the HIP head (dims=1)
    def _head_params(self):
        m, o = self.output_MLP, self.output_layer
        return [m[1].weight, m[1].bias, m[3].weight, m[3].bias, o.weight, o.bias]

    def _bufs(self, B, Tp, dev):
        key = (B, Tp, str(dev))
        cache = self.__dict__.setdefault("_head_bufs", {})
        bufs = cache.get(key)
        if bufs is None:
            from . import _lib
            C, K = self.output_layer.in_features, self.output_layer.out_features
            f = lambda *sh: th.empty(*sh, device=dev)
            nws = _lib.load().tq_classifier_head_bwd_workspace(B, C)
            bufs = dict(pooled=f(B, C), a1=f(B, C), emb=f(B, C), logits=f(B, K), dlogits=f(B, K), loss=f(1),
                        ws=th.empty(nws, dtype=th.uint8, device=dev), nws=nws,
                        grads=f(sum(p.numel() for p in self._head_params())))
            if len(cache) >= 8:   # (a handful of (batch, length) shapes live side by side: training, validation, metric batches)
                cache.clear()
            cache[key] = bufs
        return bufs

    def _head_forward(self, x, want_logits, train, seed):
        """encoder plan + tq_classifier_head_fwd into the static buffers of this shape.  Returns (emb | logits, plan, buffers)."""
        from . import _lib
        from ._lib import _p, check
        engine.require_device(x)
        x = x.contiguous()
        eng = _seq_engine(self.encoder, x)
        h = eng.forward(x, train=train, dropout_seed=seed, channels_last=True)   # (B, T', C), the output conv's own buffer
        B, Tp, C = h.shape
        bufs = self._bufs(B, Tp, x.device)
        W1, b1, W2, b2, W3, b3 = self._head_params()
        check(_lib.load().tq_classifier_head_fwd(_p(h), _p(W1), _p(b1), _p(W2), _p(b2), _p(W3), _p(b3), _p(bufs["pooled"]), _p(bufs["a1"]),
                                                 _p(bufs["emb"]), _p(bufs["logits"]) if want_logits else None, B, Tp, C, W3.shape[0],
                                                 th.cuda.current_stream(x.device).cuda_stream), "classifier head")
        return (bufs["logits"] if want_logits else bufs["emb"]), eng, bufs

    def _head_backward(self, eng, bufs, gout, want_logits):
        """tq_classifier_head_bwd: the head's parameter gradients (views of ``bufs["grads"]``, cloned; W3 / b3: None for ``embed``) and
        d loss / d h into the channels-last gradient buffer of the encoder's backward plan."""
        from . import _lib
        from ._lib import _p, check
        plan = eng.backward_plan()
        params = self._head_params()
        B, Tp, C = plan.dout_btc.shape
        flat = bufs["grads"]
        views, o = [], 0
        for p in params:
            views.append(flat[o:o + p.numel()].view_as(p))
            o += p.numel()
        dW1, db1, dW2, db2, dW3, db3 = views
        W1, _, W2, _, W3, _ = params
        check(_lib.load().tq_classifier_head_bwd(_p(gout), _p(bufs["pooled"]), _p(bufs["a1"]), _p(bufs["emb"]), _p(W1), _p(W2),
                                                 _p(W3) if want_logits else None, _p(dW3), _p(db3), _p(dW2), _p(db2), _p(dW1), _p(db1),
                                                 _p(plan.dout_btc), _p(bufs["ws"]), bufs["nws"], B, Tp, C, W3.shape[0],
                                                 th.cuda.current_stream(gout.device).cuda_stream), "classifier head backward")
        out = flat.clone()
        res, o = [], 0
        for i, p in enumerate(params):
            res.append(out[o:o + p.numel()].view_as(p) if (want_logits or i < 4) else None)
            o += p.numel()
        return res

    def _hip(self, x, want_logits):
        if th.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())):
            return _HeadFn.apply(self, x, want_logits, *self.encoder.parameters(), *self._head_params())
        train = self.training
        out, eng, _ = self._head_forward(x, want_logits, train, rng.next_dropout_seed() if train else 0)
        if eng.check_range():   # activations near the fp16 range: the plan is on bf16x3 now, repeat
            out, eng, _ = self._head_forward(x, want_logits, train, rng.next_dropout_seed() if train else 0)
        return out.clone()

    # ------------------------------------------------------------------ the reference's surface
    def embed(self, x):
        if self.encoder.dims == 1:
            return self._hip(x, False)
        h = self.encoder(x)   # batch_size x channels x ...   (stock-PyTorch family, family2d.py)
        return self.output_MLP(th.mean(h, dim=list(range(2, h.ndim))))

    def forward(self, x):
        if self.encoder.dims == 1:
            return self._hip(x, True)
        return self.output_layer(self.embed(x))

    def training_step(self, batch, batch_idx):
        loss = self.loss(self(batch["signal"]), batch["label"])
        self.log("training/loss", loss.item(), sync_dist=True)
        return loss

    def validation_step(self, batch, batch_idx):
        y = batch["label"]
        y_hat = self(batch["signal"])
        loss = self.loss(y_hat, y)
        self.log("validation/loss", loss.item(), sync_dist=True)
        values = self.metrics(y_hat, y)
        if HAVE_LIGHTNING:
            self.log_dict(self.metrics, sync_dist=True)
        else:
            for name, v in (values or {}).items():
                self.log(name, v, sync_dist=True)
        return loss

    def _fused_loss(self, y):
        """the loss is exactly what tq_cross_entropy computes: nn.CrossEntropyLoss, mean reduction, no smoothing, class-index targets"""
        ls = self.loss
        return (type(ls) is nn.CrossEntropyLoss and ls.reduction == "mean" and ls.label_smoothing == 0.0 and y.dtype == th.int64
                and y.dim() == 1)

    def step_and_backward(self, batch):
        """``training_step`` + backward without the autograd round trip (DataParallelTrainer): forward, loss and backward run back to
        back on the HIP kernels; gradients are left in ``p.grad``.  Returns (loss, [gradient tensors]).  The loss and d loss / d logits
        come from ``tq_cross_entropy`` when the loss is a plain class-index ``nn.CrossEntropyLoss``; any other loss is differentiated
        by torch on the (B, K) logits and the same HIP backward follows."""
        if self.encoder.dims == 2:
            raise NotImplementedError("DataParallelTrainer drives the 1-D HIP path; train dims=2 models with training_step() + torch.autograd")
        from . import _lib
        from ._lib import _p, check
        x, y = batch["signal"], batch["label"]
        train = self.training
        with th.no_grad():
            logits, eng, bufs = self._head_forward(x, True, train, rng.next_dropout_seed() if train else 0)
            if self._fused_loss(y):
                B, K = logits.shape
                w = self.loss.weight
                check(_lib.load().tq_cross_entropy(_p(logits), _p(y.contiguous()), _p(w), int(self.loss.ignore_index), _p(bufs["loss"]),
                                                   _p(bufs["dlogits"]), B, K, th.cuda.current_stream(x.device).cuda_stream),
                      "cross entropy")
                loss, dlogits = bufs["loss"][0].clone(), bufs["dlogits"]
            else:
                with th.enable_grad():
                    lg = logits.detach().clone().requires_grad_(True)
                    loss = self.loss(lg, y)
                    dlogits, = th.autograd.grad(loss, lg)
                loss, dlogits = loss.detach(), dlogits.contiguous().float()
            head = self._head_backward(eng, bufs, dlogits, True)
            g_enc, _ = eng.backward(None, want_dx=False, clone=True)
        grads = dict(zip((id(p) for p in self.encoder.parameters()), g_enc))
        grads.update(zip((id(p) for p in self._head_params()), head))
        flats = []
        for p in self.parameters():
            g = grads.get(id(p))
            if g is not None and p.requires_grad:
                p.grad = g
                flats.append(g)
        return loss, flats

    def configure_optimizers(self):
        optimizer = th.optim.Adam(self.parameters(), lr=self.optimizer_params["learning_rate"])
        lr_scheduler = th.optim.lr_scheduler.CosineAnnealingLR(
            optimizer, T_max=self.optimizer_params["max_steps"], eta_min=self.optimizer_params["eta_min"])
        return {"optimizer": optimizer, "lr_scheduler": {"scheduler": lr_scheduler, "interval": "step"}}
