"""Write down what the execution plans launch, so that two trees can be compared line by line (a refactor of engine.py / engine_bwd.py
must leave every launch, argument and order as it was).

    python tools/plan_listing.py LISTING.txt [OUTPUTS.pt]          (needs a GPU; run it from each tree against the SAME library build,
    python tools/plan_listing.py --diff OLD.txt NEW.txt             TQDNE_HIP_LIB=<path to libtqdne_hip.so>; then compare the two files)
    python tools/plan_listing.py --equal OLD.pt NEW.pt             (the inference outputs of every case, torch.equal)
    python tools/plan_listing.py --models LISTING.txt [OUTPUTS.pt] (the layer ABOVE the plans, see below; same --diff / --equal)
    python tools/plan_listing.py --trainer LISTING.txt [OUTPUTS.pt] (the training layer, see below; same --diff / --equal)

``--diff`` is a line diff that lets ONE kind of line move within its run: the transposed pack of an input layer's weights for the input
gradient (tq_pack_conv_weight mode 1), which only has to precede that gradient's launch: such lines are compared at the end of the run
they were made in, so their number and arguments still have to agree.

For a fixed list of small cases it builds the plan, runs one inference forward, one training forward (traced) and two backwards (plain and
traced) and writes: ``ops`` / ``ops_infer`` / ``op_bytes`` (again once the backward plan exists), the trace entries (name, FLOP, bytes) of
the forward -- the dynamic stem / head launches among them -- the backward plan's ``head_op`` / ``ops`` with ``op_flops`` / ``stem_op`` /
``dx_op``, and every call into the library made by each of those runs, in order, with the descriptors as they were armed at that moment.
Integers and floats are written as they are, a device pointer as "buf<k>+<offset>" (resolved against the tensors the plan, its store,
the model and the inputs hold; k counts first appearances within the case), a byref descriptor as its fields, a Python callable that
stands in for a launch by its name.  The second process of a full check is the same run under TQDNE_GN_FOLD=1.

``--models`` lists what the model layer (edm.py, autograd.py, consistency_model.py, diffusion.py) makes of its public calls: per case and
per call every library launch in order, with its stream (numbered by first appearance within the call) and its arguments resolved
against everything the modules, their scratch caches, their plans and the inputs hold.  A device address that resolves to nothing held
(a temporary of the call) is "tmp<k>", k by first appearance within the call.  torch.manual_seed(0) and rng.seed_rank(0) precede every
case.  In OUTPUTS.pt the inference outputs and samples carry plain names (``--equal`` demands torch.equal); losses and gradients, which
pass through the gradient kernels' atomics, carry a leading "~" (``--equal`` reports how many differ and the largest difference).

``--trainer`` lists what the training layer (trainer.py, optim.py) makes of ``DataParallelTrainer``'s public calls, per case and per call:
every library launch in order with its stream and resolved arguments, every ``torch.distributed`` collective the trainer issues (kind,
dtype, elements, asynchronous or not) where it was issued between them, and after each call the decoded rows of the fused optimizer's
step table and swap table.  In OUTPUTS.pt those tables (buffer number and offset per address) and everything of the two bare-optimizer
cases -- fixed synthetic gradients, no atomics -- carry plain names; losses, trained parameters and the norms of real backward passes
carry the "~"."""

import ctypes as C
import difflib
import gc
import os
import re
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


class Recorder:
    """Stands in for the loaded library: every entry point is wrapped ONCE (the plans compare entry points by identity) and, while
    ``log`` is a list, each call leaves (name, arguments as they are at that moment)."""

    def __init__(self, lib, protos):
        self._lib, self._fns, self.log = lib, {}, None
        # launches: int status, the stream last (the size / limit queries a plan makes while it is built are not listed)
        self._launch = {n for n, (res, args) in protos.items() if res is C.c_int and len(args) > 1 and args[-1] is C.c_void_p}
        self._ptr = {n: [t is C.c_void_p for t in args] for n, (res, args) in protos.items()}

    def __getattr__(self, name):
        fn = self._fns.get(name)
        if fn is None:
            real = getattr(self._lib, name)

            def fn(*a, _real=real, _name=name):
                if self.log is not None and _name in self._launch:
                    # (an address given as a number is marked as one; a byref descriptor under a void* parameter is copied out)
                    self.log.append((_name, [("ptr", x) if p and isinstance(x, int) else frozen(x) for x, p in zip(a, self._ptr[_name])]))
                return _real(*a)
            fn.__name__ = name
            self._fns[name] = fn
        return fn


def frozen(a):
    """an argument with every descriptor behind it copied out: int | float | None | ("ptr", address) | ("struct", [(field, value)])"""
    if hasattr(a, "_obj"):          # ctypes.byref(...)
        a = a._obj
    if isinstance(a, C.Structure):
        return ("struct", [(f[0], ("ptr", getattr(a, f[0])) if f[1] is C.c_void_p else frozen(getattr(a, f[0]))) for f in a._fields_])
    if isinstance(a, C._Pointer):
        return frozen(a.contents) if a else None
    return a


def stream_of(args):
    s = args[-1]
    return (s[1] if isinstance(s, tuple) else s) or 0


class Names:
    """device address -> "buf<k>+<offset>" against a set of storages; k in order of first appearance.  ``tmp`` (a dict): an address
    that is known to be one (an argument or descriptor field of pointer type) and lies in no storage is "tmp<k>" instead of a number."""

    def __init__(self):
        self.ranges, self.k, self.seen, self.tmp = {}, {}, set(), None

    def gather(self, o, depth=0):
        if id(o) in self.seen or depth > 8:
            return
        self.seen.add(id(o))
        if isinstance(o, torch.Tensor):
            self.seen.discard(id(o))   # (views are short-lived: their ids get reused)
            if o.is_cuda:
                st = o.untyped_storage()
                self.ranges[st.data_ptr()] = max(self.ranges.get(st.data_ptr(), 0), st.nbytes())
        elif isinstance(o, torch.nn.Module):
            for t in list(o.parameters()) + list(o.buffers()):
                self.gather(t, depth + 1)
            for v in o.__dict__.get("_packed_stores", {}).values():
                self.gather(v, depth + 1)
        elif isinstance(o, dict):
            for v in o.values():
                self.gather(v, depth + 1)
        elif isinstance(o, (list, tuple, set)):
            for v in o:
                self.gather(v, depth + 1)
        elif type(o).__module__.startswith("tqdne_amd"):
            for n in list(getattr(o, "__dict__", ())) + [s for c in type(o).__mro__ for s in getattr(c, "__slots__", ())]:
                self.gather(getattr(o, n, None), depth + 1)

    def arg(self, a, ptr=False):
        if isinstance(a, tuple) and a and a[0] == "struct":
            return "{" + " ".join(f"{n}={self.arg(v)}" for n, v in a[1]) + "}"
        if isinstance(a, tuple) and a and a[0] == "ptr":
            return self.arg(a[1], True)
        if isinstance(a, int) and a >= 4096:
            for base, size in self.ranges.items():
                if base <= a < base + max(size, 1):
                    k = self.k.setdefault(base, len(self.k))
                    return f"buf{k}+{a - base}"
            if ptr and self.tmp is not None:
                return f"tmp{self.tmp.setdefault(a, len(self.tmp))}"
        return repr(a)

    def call(self, fn, args):
        return f"{fn if isinstance(fn, str) else fn.__name__}({', '.join(self.arg(frozen(a)) for a in args)})"


def perturbed(mod, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in mod.parameters():
            p.add_(0.02 * torch.randn(p.shape, generator=g))
    return mod.cuda().eval()


def rnd(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).cuda()


def cases():
    """(title, build() -> (plan, forward(train, infer), backward()))"""
    from tqdne_amd import Decoder, Encoder, UNetModel, engine, tiny_1d_unet_config
    micro = dict(model_channels=32, channel_mult=(1, 2), num_res_blocks=1, attention_resolutions=(2,), num_heads=4, conv_kernel_size=5,
                 dims=1, cond_features=5, dropout=0.1)
    coder = dict(model_channels=32, num_res_blocks=1, attention_resolutions=(), channel_mult=(1, 2), conv_kernel_size=3, dims=1, dropout=0.1)

    def unet(cfg, B=2, T=256, c1=0, solo=True, edm=False, bf16x3=False, want_dx=False, cout=None):
        def build():
            torch.manual_seed(0)
            m = perturbed(UNetModel(**cfg), 1)
            eng = engine.UNetEngine(m, B, T, torch.device("cuda", 0), solo=solo)
            if bf16x3:
                eng._set_scheme_bf16x3()
            x, t = rnd(2, B, cfg["in_channels"] - c1, T), rnd(3, B).abs() + 0.1
            cond = rnd(4, B, cfg["cond_features"]) if cfg.get("cond_features") else None
            kw = dict(cond_x=rnd(5, B, c1, T)) if c1 else {}
            sc = dict(in_scale=rnd(6, B).abs() + 0.5, c_out=rnd(7, B).abs() + 0.5) if edm else {}
            if edm and cfg["out_channels"] == x.shape[1]:
                sc.update(c_skip=rnd(8, B).abs(), skip_src=x)
            dpred = rnd(9, B, cfg["out_channels"], T)
            held = [x, t, cond, kw, sc, dpred]
            fwd = lambda train, infer: eng.forward(x, t, cond, train=train, dropout_seed=11, infer=infer, **sc, **kw)
            bwd = lambda: eng.backward(dpred, torch.tensor(0.5, device="cuda"), want_dx=want_dx)
            return m, eng, fwd, bwd, held
        return build

    def seq(cls, cfg, B=2, T=200):
        def build():
            torch.manual_seed(0)
            m = perturbed(cls(**cfg), 1)
            eng = engine.SeqEngine(m, B, T, torch.device("cuda", 0))
            x = rnd(2, B, cfg["in_channels"], T)
            dout = rnd(9, *eng.out_nct.shape)
            fwd = lambda train, infer: eng.forward(x, train=train, dropout_seed=11)
            bwd = lambda: eng.backward(dout, want_dx=True)
            return m, eng, fwd, bwd, [x, dout]
        return build

    tiny = tiny_1d_unet_config()
    heads = dict(micro, attention_resolutions=(1, 2), cond_features=None)
    return [
        ("1 tiny UNet, 3 channels, EDM scales, want_dx", unet(tiny, edm=True, want_dx=True)),
        ("2 tiny UNet, 16 -> 16 channels (generic stem gradient over a copy)", unet(tiny_1d_unet_config(16, 16), want_dx=True)),
        ("3 wide stem (16 + 16 cond_x) and wide head (24)", unet(dict(micro, in_channels=32, out_channels=24), c1=16, edm=True, want_dx=True)),
        ("4 use_checkpoint", unet(dict(micro, in_channels=3, out_channels=3, use_checkpoint=True))),
        ("5 conv_resample=False, cond_emb_scale", unet(dict(micro, in_channels=3, out_channels=3, conv_resample=False, cond_features=1,
                                                            cond_emb_scale=2.0))),
        ("6a attention heads of 8 and 16 channels", unet(dict(heads, in_channels=3, out_channels=3))),
        ("6b attention heads of 64 and 128 channels", unet(dict(heads, model_channels=64, num_heads=1, in_channels=3, out_channels=3))),
        ("6c attention heads of 32 channels", unet(dict(micro, model_channels=64, in_channels=3, out_channels=3))),
        ("7 B = 4 (small tile, folded GroupNorm)", unet(tiny, B=4)),
        ("8a B = 16, T = 1024, solo", unet(dict(heads, in_channels=3, out_channels=3), B=16, T=1024)),
        ("8b B = 16, T = 1024, a lane", unet(dict(heads, in_channels=3, out_channels=3), B=16, T=1024, solo=False)),
        ("9 Encoder 3 -> 32", seq(Encoder, dict(coder, in_channels=3, out_channels=32))),
        ("10 Decoder 16 -> 3", seq(Decoder, dict(coder, in_channels=16, out_channels=3))),
        ("11 Encoder, 24 signal channels", seq(Encoder, dict(coder, in_channels=24, out_channels=32))),
        ("12 case 1 after _set_scheme_bf16x3()", unet(tiny, edm=True, want_dx=True, bf16x3=True)),
    ]


def listing(out, outputs):
    from tqdne_amd import _lib, engine
    rec = _lib._LIB = Recorder(_lib.load(), _lib._PROTOS)
    for title, build in cases():
        out.write(f"==== case {title}\n")
        m, eng, fwd, bwd, held = build()
        names = Names()

        def known():
            names.seen.clear()
            for o in (m, eng, eng._bwd, held, list(engine._PACK_TABLES.values())):
                names.gather(o)

        def static(tag, ops, extra=lambda i: ""):
            known()
            out.write(f"-- {tag}\n")
            for i, op in enumerate(ops):
                out.write(f"{i:4d} {op[2]}{extra(i)}: {names.call(op[0], op[1])}\n")

        def run(tag, f):
            rec.log = []
            y = f()
            held.append(y)   # (a fresh tensor a launch wrote, the input gradient, has a name only while somebody holds it)
            torch.cuda.synchronize()
            log, rec.log = rec.log, None
            known()
            out.write(f"-- calls: {tag}\n")
            streams = {}
            for name, args in log:
                s = stream_of(args)   # (every launch takes the stream last; the ones of this process in order of appearance)
                out.write(f"     {names.call(name, args[:-1])} on stream {streams.setdefault(s, len(streams))}\n")
            return y

        def fwd_lists(tag):
            static("ops" + tag, eng.ops, lambda i: f" flop={eng.ops[i][3]} bytes={eng.op_bytes[i]}")
            static("ops_infer" + tag, eng.ops_infer, lambda i: f" flop={eng.ops_infer[i][3]}")
        fwd_lists("")
        outputs[title] = run("inference forward", lambda: fwd(False, True)).clone().cpu()
        eng._trace = []
        run("training forward (traced)", lambda: fwd(True, False))
        out.write("-- trace of the training forward\n")
        for what, fl, nb, _a, _b in eng._trace:
            out.write(f"     {what} flop={fl} bytes={nb}\n")
        eng._trace = None
        run("training forward", lambda: fwd(True, False))
        run("backward", bwd)
        b = eng._bwd
        b._trace = []
        run("training forward, block K / V kept", lambda: fwd(True, False))
        run("backward (traced)", bwd)
        out.write("-- trace of the backward\n")
        for what, fl, nb, _a, _b in b._trace:
            out.write(f"     {what} flop={fl} bytes={nb}\n")
        b._trace = None
        fwd_lists(" once the backward plan exists")
        for tag in ("head_op", "stem_op", "dx_op"):
            op = getattr(b, tag, None)
            static("backward " + tag, [op] if op is not None else [])
        static("backward ops", b.ops, lambda i: f" flop={b.op_flops.get(i, 0)}")
        out.write(f"-- scheme={eng.scheme} wide_stem={eng.wide_stem} n_grad={b.n_grad}\n")


def model_cases():
    """(title, build() -> (modules, held, [(tag, call() -> {name: tensor to save})])) -- only names both sides of a refactor of the model
    layer have: forward, step_with_noise, step_and_backward, sample_deterministically, sample_stochastically, sample_from,
    LithningConsistencyModel.step, LightningDDMP.step_with_noise, autograd.edm_loss_and_grads"""
    from tqdne_amd import DDPMScheduler, LightningDDMP, LightningEDM, LithningConsistencyModel, UNetModel, autograd, tiny_1d_unet_config
    micro = dict(model_channels=32, channel_mult=(1, 2), num_res_blocks=1, attention_resolutions=(2,), num_heads=4, conv_kernel_size=5,
                 dims=1, cond_features=5, dropout=0.1)
    wide = dict(micro, in_channels=32, out_channels=16)          # 16 + 16 input channels: the wide stem concatenates the signal
    tiny, narrow = tiny_1d_unet_config(), tiny_1d_unet_config(6, 3)   # narrow: 3 + 3 channels through tq_concat_scale
    opt = {"learning_rate": 1e-4, "max_steps": 10, "eta_min": 0.0}
    T = 256

    def inputs(cfg, B, c1):
        cond = rnd(4, B, cfg["cond_features"]) if cfg.get("cond_features") else None
        return rnd(2, B, cfg["in_channels"] - c1, T), rnd(3, B).abs() + 0.1, (rnd(5, B, c1, T) if c1 else None), cond

    def grads(m):
        return torch.cat([p.grad.flatten() for p in m.parameters() if p.grad is not None])

    def env(name, value, f):
        def g():
            os.environ[name] = value
            try:
                return f()
            finally:
                del os.environ[name]
        return g

    def edm(cfg, c1=0, B=2, train=False):
        m = perturbed(LightningEDM(cfg, opt, num_sampling_steps=3), 1).train(train)
        return (m,) + inputs(cfg, B, c1)

    def edm_forward(cfg, c1):
        def build():
            m, x, sigma, cs, cond = edm(cfg, c1)

            def call():
                with torch.no_grad():
                    return {"y": m(x, sigma, cs, cond)}
            return [m], [x, sigma, cs, cond], [("forward under no_grad", call)]
        return build

    def edm_forward_grad(cfg, c1, train):
        def build():
            m, x, sigma, cs, cond = edm(cfg, c1, train=train)
            G = rnd(9, *x.shape)

            def call():
                m.zero_grad(set_to_none=True)
                xg = x.clone().requires_grad_(True)
                y = m(xg, sigma, cs, cond)
                (y * G).sum().backward()
                return {"~y": y.detach(), "~dx": xg.grad, "~grads": grads(m)}
            return [m], [x, sigma, cs, cond, G], [("forward with grad, backward", call)]
        return build

    def edm_step(cfg, c1, how, B=2, lanes=1):
        def build():
            m, x, _, cs, cond = edm(cfg, c1, B, train=True)
            eps, noise = rnd(6, B), rnd(7, *x.shape)
            batch = {k: v for k, v in (("signal", x), ("cond_signal", cs), ("cond", cond)) if v is not None}

            def call():
                m.zero_grad(set_to_none=True)
                if how == "step_with_noise":
                    loss = m.step_with_noise(x, eps, noise, cond=cond, cond_sample=cs)
                    loss.backward()
                elif how == "step_and_backward":
                    loss, _ = m.step_and_backward(batch)
                else:
                    loss, _ = autograd.edm_loss_and_grads(m, x, eps, noise, cond, cs, lanes=lanes)
                return {"~loss": loss.detach(), "~grads": grads(m)}
            if how == "step_and_backward" and lanes > 1:
                call = env("TQDNE_TRAIN_LANES", str(lanes), call)
            return [m], [x, cs, cond, eps, noise], [(f"{how}, lanes={lanes}", call), (f"{how} again", call)]
        return build

    def edm_sample(cfg, c1, B, churn=False, repeat=1, **kw):
        def build():
            m, x, _, cs, cond = edm(cfg, c1, B)
            sigmas = m.edm.sampling_sigmas(3).cuda()
            start = (rnd(8, *x.shape).double() * sigmas[0]).contiguous()
            if churn:
                kw["churn_noises"] = [rnd(20 + i, *x.shape).double() for i in range(3)]
            f = m.sample_stochastically if churn else m.sample_deterministically
            call = lambda: {"sample": f(start, sigmas, cs, cond, **kw)}
            return [m], [start, sigmas, cs, cond, kw], [(f"call {i}", call) for i in range(repeat)]
        return build

    def cm(cfg, c1, what, B=2):
        def build():
            m = perturbed(LithningConsistencyModel(UNetModel(**cfg)), 1)
            x, sigma, cs, cond = inputs(cfg, B, c1)
            us = [torch.rand(x.shape, generator=torch.Generator().manual_seed(30 + i)).cuda() for i in range(2)]

            def forward():
                with torch.no_grad():
                    return {"y": m(x, sigma, cs, cond)}

            def step():
                m.zero_grad(set_to_none=True)
                m.step({k: v for k, v in (("signal", x), ("cond_signal", cs), ("cond", cond)) if v is not None}).backward()
                return {"~grads": grads(m)}
            call = {"forward": forward, "lanes": env("TQDNE_CM_LANES", "2", forward), "step": step,
                    "sample_from": lambda: {"sample": m.sample_from(x, [2.0, 0.5], us, cs, cond)}}[what]
            m.train(what == "step")
            m.max_steps = 1000   # (no trainer: the iCT schedule reads the module's own attribute)
            return [m], [x, sigma, cs, cond, us], [(what, call)]
        return build

    def ddpm(cfg, c1):
        def build():
            m = perturbed(LightningDDMP(UNetModel(**cfg), DDPMScheduler(), opt, cond_signal_input=bool(c1)), 1).train()
            x, _, cs, _ = inputs(cfg, 2, c1)
            noise, t = rnd(7, *x.shape), torch.tensor([10, 700]).cuda()

            def call():
                m.zero_grad(set_to_none=True)
                loss = m.step_with_noise({"signal": x, "cond_signal": cs}, noise, t)
                loss.backward()
                return {"~loss": loss.detach(), "~grads": grads(m)}
            return [m], [x, cs, noise, t], [("step_with_noise, backward", call)]
        return build

    return [
        ("1a EDM forward, plain", edm_forward(tiny, 0)),
        ("1b EDM forward, cond_sample on a narrow stem (3 + 3)", edm_forward(narrow, 3)),
        ("1c EDM forward, cond_sample on a wide stem (16 + 16)", edm_forward(wide, 16)),
        ("2a EDM forward with grad and backward, narrow concat, eval mode", edm_forward_grad(narrow, 3, False)),
        ("2b EDM forward with grad and backward, wide stem, train mode", edm_forward_grad(wide, 16, True)),
        ("3a step_with_noise and loss.backward()", edm_step(tiny, 0, "step_with_noise")),
        ("3b step_with_noise and loss.backward(), wide stem", edm_step(wide, 16, "step_with_noise")),
        ("4a step_and_backward, one lane", edm_step(tiny, 0, "step_and_backward")),
        ("4b step_and_backward, B = 16 on two lanes", edm_step(tiny, 0, "step_and_backward", B=16, lanes=2)),
        ("4c edm_loss_and_grads, B = 16 on two lanes, narrow concat", edm_step(narrow, 3, "edm_loss_and_grads", B=16, lanes=2)),
        ("5a sample_deterministically, one lane", edm_sample(tiny, 0, 2)),
        ("5b sample_deterministically, one lane, wide stem", edm_sample(wide, 16, 2)),
        ("5c sample_deterministically, B = 16 on two lanes", edm_sample(tiny, 0, 16, lanes=2)),
        ("5d sample_deterministically, B = 16 on two lanes, narrow concat", edm_sample(narrow, 3, 16, lanes=2)),
        ("5e sample_deterministically, use_graph='denoiser', capture and two replays", edm_sample(tiny, 0, 2, repeat=3, use_graph="denoiser")),
        ("5f sample_deterministically, use_graph=True, capture and two replays", edm_sample(narrow, 3, 2, repeat=3, use_graph=True)),
        ("6a sample_stochastically, given noises, one lane", edm_sample(narrow, 3, 2, churn=True, lanes=1)),
        ("6b sample_stochastically, given noises, B = 16 on two lanes", edm_sample(tiny, 0, 16, churn=True, lanes=2)),
        ("7a consistency forward, plain", cm(tiny, 0, "forward")),
        ("7b consistency forward, narrow concat", cm(narrow, 3, "forward")),
        ("7c consistency forward, wide stem", cm(wide, 16, "forward")),
        ("7d consistency forward, B = 16, TQDNE_CM_LANES=2", cm(narrow, 3, "lanes", B=16)),
        ("7e consistency sample_from, two sigmas", cm(tiny, 0, "sample_from")),
        ("7f consistency step and backward, narrow concat", cm(narrow, 3, "step")),
        ("8a DDPM step_with_noise and backward", ddpm(tiny, 0)),
        ("8b DDPM step_with_noise and backward, cond_signal_input", ddpm(narrow, 3)),
    ]


def model_listing(out, outputs):
    from tqdne_amd import _lib, engine, rng
    rec = _lib._LIB = Recorder(_lib.load(), _lib._PROTOS)
    for title, build in model_cases():
        out.write(f"==== case {title}\n")
        # (every case starts from an empty allocator: whether a temporary's address is later reused by something held, and so gets a
        # name, then depends on the case alone, not on what earlier cases left cached)
        mods = held = calls = names = None
        gc.collect()
        torch.cuda.empty_cache()
        torch.manual_seed(0)
        rng.seed_rank(0)
        mods, held, calls = build()
        names = Names()
        for tag, call in calls:
            rec.log = []
            res = call()
            torch.cuda.synchronize()
            log, rec.log = rec.log, None
            held.append(res)
            names.seen.clear()
            names.tmp = {}
            for m in mods:   # (a module hands its parameters over; its scratch cache and its network's plans are looked up by name)
                nets = [n for n in (getattr(m, "unet", None), getattr(m, "net", None)) if n is not None]
                plans = [e for n in nets for e in n._engine_cache.values()]
                for o in [m, *nets, getattr(m, "_scal", None), *plans, *(e._bwd for e in plans)]:
                    names.gather(o)
            names.gather(held)
            names.gather(list(engine._PACK_TABLES.values()))
            out.write(f"-- calls: {tag}\n")
            streams = {}
            for name, args in log:
                s = stream_of(args)
                out.write(f"     {names.call(name, args[:-1])} on stream {streams.setdefault(s, len(streams))}\n")
            for k, v in res.items():
                outputs[f"{'~' if k[0] == '~' else ''}{title} / {tag} / {k.lstrip('~')}"] = v.detach().clone().cpu()


class Collectives:
    """``dist.all_reduce`` / ``dist.broadcast`` wrapped for the duration: while the recorder logs, each call leaves ("@kind", [dtype,
    elements, async?]) in its log, between the launches it was issued between."""

    def __init__(self, rec):
        self.rec = rec

    def __enter__(self):
        import torch.distributed as dist
        self.saved = {k: getattr(dist, k) for k in ("all_reduce", "broadcast")}
        for kind, real in self.saved.items():
            def f(t, *a, _kind=kind, _real=real, **k):
                if self.rec.log is not None:
                    self.rec.log.append(("@" + _kind, [str(t.dtype), t.numel(), bool(k.get("async_op", False))]))
                return _real(t, *a, **k)
            setattr(dist, kind, f)

    def __exit__(self, *exc):
        import torch.distributed as dist
        for kind, real in self.saved.items():
            setattr(dist, kind, real)


def trainer_cases():
    """(title, build() -> (roots, optimizers, [(tag, call() -> {name: tensor to save})])): ``roots`` is what the addresses are resolved
    against (trainers, modules, inputs), ``optimizers`` the fused optimizers whose step and swap tables are written after every call;
    a call may append to both.  Only names both sides of a refactor of the training layer have."""
    import tempfile

    from tqdne_amd import LightningAutoencoder, LightningEDM, LithningConsistencyModel, UNetModel, tiny_1d_unet_config
    from tqdne_amd.optim import FusedAdamEMA, FusedRAdamEMA
    from tqdne_amd.trainer import DataParallelTrainer
    tiny = tiny_1d_unet_config()
    micro = dict(in_channels=3, out_channels=3, model_channels=32, channel_mult=(1, 2), num_res_blocks=1, attention_resolutions=(2,),
                 num_heads=4, conv_kernel_size=5, dims=1, cond_features=5, dropout=0.1)
    coder = dict(model_channels=32, num_res_blocks=1, attention_resolutions=(), channel_mult=(1, 2), conv_kernel_size=3, dims=1, dropout=0.1)
    opt = {"learning_rate": 1e-3, "max_steps": 10, "eta_min": 0.0}
    B, T = 2, 256

    def module(kind, cfg=micro):
        if kind == "edm":
            return perturbed(LightningEDM(cfg, opt, num_sampling_steps=3), 1).train()
        if kind == "cm":
            return perturbed(LithningConsistencyModel(UNetModel(**cfg), initial_timesteps=10, final_timesteps=40), 1).train()
        return perturbed(LightningAutoencoder(dict(coder, in_channels=3, out_channels=32), dict(coder, in_channels=16, out_channels=3), opt), 1).train()

    def batch(seed=2, cond=True):
        return dict({"signal": 0.5 * rnd(seed, B, 3, T)}, **({"cond": rnd(seed + 100, B, 5)} if cond else {}))

    def flat(m):
        return torch.cat([p.detach().flatten() for p in m.parameters()])

    def steps(tr, b, n=3, parameters=True):
        def step():
            res = {"~loss": tr.train_step(b).detach()}
            if tr.last_grad_norm is not None:
                res["~grad norm"] = tr.last_grad_norm.detach().clone()
            return res
        return [(f"train_step {i + 1}", step) for i in range(n)] + [("parameters", lambda: {"~parameters": flat(tr.module)})][:parameters]

    def train(kind, cfg=micro, **kw):
        def build():
            m, b = module(kind, cfg), batch(cond=kind != "ae" and bool(cfg["cond_features"]))
            tr = DataParallelTrainer(m, world_size=1, **kw)
            return [tr, b], [tr.optimizer] if tr.fused else [], steps(tr, b, parameters=cfg is not tiny)   # (3.5 M of them)
        return build

    def evaluate():
        def build():
            m, b = module("edm"), batch()
            tr = DataParallelTrainer(m, world_size=1, ema_decay=0.9)
            x, sigma = rnd(12, B, 3, T), rnd(13, B).abs() + 0.1

            def forward():
                with tr.ema_weights(), torch.no_grad():
                    return {"~y on the EMA weights": m(x, sigma, None, b["cond"])}
            return [tr, b, x, sigma], [tr.optimizer], steps(tr, b, 1)[:1] + [
                ("validate on two batches", lambda: {"~validation loss": tr.validate([batch(10), batch(11)])}),
                ("inference forward inside ema_weights()", forward)]
        return build

    def resume():
        def build():
            m, b = module("edm"), batch()
            tr = DataParallelTrainer(m, world_size=1, ema_decay=0.9)
            path = os.path.join(tempfile.mkdtemp(), "listing.ckpt")
            roots, opts = [tr, b], [tr.optimizer]
            tr2 = []

            def load():
                tr2.append(DataParallelTrainer(module("edm"), world_size=1, ema_decay=0.9))
                roots.append(tr2[0])
                opts.append(tr2[0].optimizer)
                tr2[0].load_checkpoint(path)
                return {}
            return roots, opts, steps(tr, b, 1)[:1] + [
                ("save_checkpoint", lambda: tr.save_checkpoint(path) or {}), ("load_checkpoint into a fresh trainer", load),
                ("train_step 2 of the fresh trainer", lambda: {"~loss": tr2[0].train_step(b).detach()}),
                ("parameters", lambda: {"~parameters": flat(tr2[0].module)})]
        return build

    def bare(cls, **kw):
        """the optimizer alone on fixed synthetic gradients: no atomics anywhere, every saved tensor is compared with torch.equal"""
        def build():
            sizes = [1, 3, 4, 5, 4095, 4096, 4097, 2 * 4096 + 3, 7]
            ps = [torch.nn.Parameter(rnd(40 + i, n)) for i, n in enumerate(sizes)]
            o = cls([(f"p{i}", p) for i, p in enumerate(ps)], lr=1e-3, ema_decay=0.9, **kw)
            for i, p in enumerate(ps[:-1]):   # (the last parameter never has a gradient: the step's table leaves it out)
                p.grad = rnd(60 + i, *p.shape)

            def state():
                return {"parameters": torch.cat([p.detach().flatten() for p in ps]), "m": o._m.clone(), "v": o._v.clone(), "ema": o._ema.clone()}

            def step(**skw):
                def call():
                    o.step(**skw)
                    return dict(state(), **({"grad norm": o.last_grad_norm.clone()} if skw.get("max_grad_norm") or skw.get("track_grad_norm") else {}))
                return call
            return [o, ps, [p.grad for p in ps]], [o], [("step 1", step()), ("step 2, max_grad_norm", step(max_grad_norm=0.5, grad_scale=0.5)),
                                  ("step 3, clip_value and track_grad_norm", step(clip_value=0.01, track_grad_norm=True)),
                                  ("swap_ema", lambda: o.swap_ema() or state()), ("swap_ema back", lambda: o.swap_ema() or state())]
        return build

    ema = dict(ema_decay=0.9)
    forced = dict(ema, force_exchange=True, bucket_bytes=64 << 10)
    return [
        ("1a EDM on the tiny UNet, fused Adam + EMA", train("edm", tiny, **ema)),
        ("1b consistency model, fused RAdam + EMA, max_steps=6", train("cm", max_steps=6, **ema)),
        ("1c autoencoder, fused AdamW + EMA", train("ae", **ema)),
        ("2a EDM, gradient_clip_val by norm", train("edm", gradient_clip_val=0.05, **ema)),
        ("2b EDM, gradient_clip_val by value", train("edm", gradient_clip_val=0.01, gradient_clip_algorithm="value", **ema)),
        ("2c EDM, track_grad_norm alone", train("edm", track_grad_norm=True, **ema)),
        ("3a EDM, force_exchange over one gloo rank, overlap=True", train("edm", overlap=True, **forced)),
        ("3b EDM, force_exchange over one gloo rank, overlap=False", train("edm", overlap=False, **forced)),
        ("4 validate and ema_weights()", evaluate()),
        ("5 save_checkpoint, load_checkpoint into a fresh trainer, one step", resume()),
        ("6 EDM, fused_optimizer=False + EMA (plan launches and collectives only)", train("edm", fused_optimizer=False, **ema)),
        ("7a FusedAdamEMA alone, weight_decay", bare(FusedAdamEMA, weight_decay=1e-2)),
        ("7b FusedRAdamEMA alone", bare(FusedRAdamEMA)),
    ]


def trainer_listing(out, outputs):
    import torch.distributed as dist

    from tqdne_amd import _lib, engine, rng
    from tqdne_amd._lib import TqAdamChunk
    rec = _lib._LIB = Recorder(_lib.load(), _lib._PROTOS)
    dist.init_process_group("gloo", store=dist.HashStore(), rank=0, world_size=1)   # (for the force_exchange cases)

    def gather_all(names, roots):
        names.seen.clear()
        names.ranges.clear()   # (only what is held NOW: the range of a freed storage would claim whatever is allocated there next)
        for o in roots:
            names.gather(o)
            m = getattr(o, "module", None)
            if isinstance(m, torch.nn.Module):   # (a module hands its parameters over; gradients, scratch cache and plans are looked up)
                names.gather([p.grad for p in m.parameters()])
                names.gather(getattr(m, "_scal", None))
                for sm in m.modules():
                    for e in sm.__dict__.get("_engine_cache", {}).values():
                        names.gather(e)
                        names.gather(e._bwd)
        names.gather(list(engine._PACK_TABLES.values()))

    def table(names, t, n):
        """decoded rows of a device chunk table, addresses resolved; (lines, rows as integers: buffer number | -1, offset, ..., n)"""
        if t is None or not n:
            return [], torch.zeros(0, 11, dtype=torch.int64)
        lines, rows = [], []
        for r in (TqAdamChunk * n).from_buffer_copy(bytes(t.cpu().tolist())):
            txt = [names.arg(("ptr", getattr(r, f) or 0)) for f in ("p", "g", "m", "v", "ema")]
            lines.append(" ".join(f"{f}={x}" for f, x in zip("p g m v ema".split(), txt)) + f" n={r.n}")
            where = [re.fullmatch(r"buf(\d+)\+(\d+)", x) for x in txt]
            rows.append([int(v) for w in where for v in (w.groups() if w else (-1, 0))] + [r.n])
        return lines, torch.tensor(rows, dtype=torch.int64)

    with Collectives(rec):
        for title, build in trainer_cases():
            out.write(f"==== case {title}\n")
            roots = opts = calls = names = None   # (every case starts from an empty allocator, see model_listing)
            gc.collect()
            torch.cuda.empty_cache()
            torch.manual_seed(0)
            rng.seed_rank(0)
            rec.log = []
            roots, opts, calls = build()          # (the constructor's broadcast belongs to the listing)
            names, written = Names(), {}
            for tag, call in [("construction", dict)] + calls:
                if tag != "construction":
                    rec.log = []
                res = call()
                torch.cuda.synchronize()
                log, rec.log = rec.log, None
                roots.append(res)
                names.tmp = {}
                gather_all(names, roots)
                out.write(f"-- calls: {tag}\n")
                streams = {}
                for name, args in log:
                    if name[0] == "@":
                        out.write(f"     collective {name[1:]} of {args[1]} x {args[0]}, async_op={args[2]}\n")
                    else:
                        s = stream_of(args)
                        if name == "tq_pack_jobs":   # (its job table is uploaded for this one launch and freed: whatever is allocated
                            args = [0] + args[1:]    # at that address later in the call must not lend it its name)
                        out.write(f"     {names.call(name, args[:-1])} on stream {streams.setdefault(s, len(streams))}\n")
                for i, o in enumerate(opts):
                    for what, t, n in (("step", o._table, getattr(o, "_n_chunks", 0)), ("swap", o._swap_table, getattr(o, "_swap_chunks", 0))):
                        lines, rows = table(names, t, n)
                        same = written.get((i, what)) == lines   # (written out when it changes, compared after every call)
                        out.write(f"-- optimizer {i}, {what} table: {len(lines)} rows{', as written above' if same and lines else ''}\n")
                        if not same:
                            out.writelines(f"     {l}\n" for l in lines)
                            written[i, what] = lines
                            outputs[f"{title} / {tag} / optimizer {i} {what} table"] = rows
                for k, v in res.items():
                    outputs[f"{'~' if k[0] == '~' else ''}{title} / {tag} / {k.lstrip('~')}"] = v.detach().clone().cpu()
    dist.destroy_process_group()


def movable_last(path):
    """the listing with the lines that may move (see --diff) put at the end of the run they belong to -- so a run that lost or gained one
    still differs -- and the buffers renumbered in that order of appearance within each case"""
    out, held, k = [], [], {}

    def emit(line):
        out.append(re.sub(r"buf(\d+)", lambda g: "buf%d" % k.setdefault(g.group(1), len(k)), line))
    for line in open(path):
        if line.startswith(("==== case", "-- ")):   # (a new section: the run before it is complete)
            for h in held:
                emit("     anywhere in this run:" + h.lstrip(" "))
            held = []
        if line.startswith("==== case"):
            k = {}
        if re.search(r"tq_pack_conv_weight\(buf\d+\+0, \d+, \d+, \d+, 1, buf\d+\+0\)", line):
            held.append(line)
        else:
            emit(line)
    return out + held


if __name__ == "__main__":
    if sys.argv[1] == "--diff":
        a, b = movable_last(sys.argv[2]), movable_last(sys.argv[3])
        d = list(difflib.unified_diff(a, b, sys.argv[2], sys.argv[3], n=0))
        sys.stdout.writelines(d)
        print(f"{len(a)} / {len(b)} lines, {sum(1 for x in d if x[0] in '+-' and x[:3] not in ('+++', '---'))} differ")
        sys.exit(1 if d else 0)
    if sys.argv[1] == "--equal":
        a, b = torch.load(sys.argv[2]), torch.load(sys.argv[3])
        exact = [k for k in set(a) | set(b) if k[0] != "~"]
        bad = sorted(k for k in exact if k not in a or k not in b or not torch.equal(a[k], b[k]))
        print(f"{len(exact)} inference outputs, {len(bad)} differ", *bad, sep="\n  ")
        loose = sorted(k for k in a if k[0] == "~" and k in b)   # (through the gradient kernels' atomics: reported, not judged)
        if loose:
            diff = {k: float((a[k].double() - b[k].double()).abs().max()) for k in loose if not torch.equal(a[k], b[k])}
            print(f"{len(loose)} losses / gradients, {len(diff)} not bit-equal, largest difference {max(diff.values(), default=0.0):.3e}")
        sys.exit(1 if bad else 0)
    mode = {"--models": model_listing, "--trainer": trainer_listing}.get(sys.argv[1])
    argv = sys.argv[2:] if mode else sys.argv[1:]
    outs = {}
    with open(argv[0], "w") as f:
        (mode or listing)(f, outs)
    if len(argv) > 1:
        torch.save(outs, argv[1])
