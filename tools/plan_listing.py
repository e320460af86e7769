"""Write down what the execution plans launch, so that two trees can be compared line by line (a refactor of engine.py / engine_bwd.py
must leave every launch, argument and order as it was).

    python tools/plan_listing.py LISTING.txt [OUTPUTS.pt]          (needs a GPU; run it from each tree against the SAME library build,
    python tools/plan_listing.py --diff OLD.txt NEW.txt             TQDNE_HIP_LIB=<path to libtqdne_hip.so>; then compare the two files)
    python tools/plan_listing.py --equal OLD.pt NEW.pt             (the inference outputs of every case, torch.equal)

``--diff`` is a line diff that lets ONE kind of line move within its run: the transposed pack of an input layer's weights for the input
gradient (tq_pack_conv_weight mode 1), which only has to precede that gradient's launch: such lines are compared at the end of the run
they were made in, so their number and arguments still have to agree.

For a fixed list of small cases it builds the plan, runs one inference forward, one training forward (traced) and two backwards (plain and
traced) and writes: ``ops`` / ``ops_infer`` / ``op_bytes`` (again once the backward plan exists), the trace entries (name, FLOP, bytes) of
the forward -- the dynamic stem / head launches among them -- the backward plan's ``head_op`` / ``ops`` with ``op_flops`` / ``stem_op`` /
``dx_op``, and every call into the library made by each of those runs, in order, with the descriptors as they were armed at that moment.
Integers and floats are written as they are, a device pointer as "buf<k>+<offset>" (resolved against the tensors the plan, its store,
the model and the inputs hold; k counts first appearances within the case), a byref descriptor as its fields, a Python callable that
stands in for a launch by its name.  The second process of a full check is the same run under TQDNE_GN_FOLD=1."""

import ctypes as C
import difflib
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

    def __getattr__(self, name):
        fn = self._fns.get(name)
        if fn is None:
            real = getattr(self._lib, name)

            def fn(*a, _real=real, _name=name):
                if self.log is not None and _name in self._launch:
                    self.log.append((_name, [frozen(x) for x in a]))
                return _real(*a)
            fn.__name__ = name
            self._fns[name] = fn
        return fn


def frozen(a):
    """an argument with every descriptor behind it copied out: int | float | None | ("struct", [(field, value)])"""
    if hasattr(a, "_obj"):          # ctypes.byref(...)
        a = a._obj
    if isinstance(a, C.Structure):
        return ("struct", [(f[0], frozen(getattr(a, f[0]))) for f in a._fields_])
    if isinstance(a, C._Pointer):
        return frozen(a.contents) if a else None
    return a


class Names:
    """device address -> "buf<k>+<offset>" against a set of storages; k in order of first appearance"""

    def __init__(self):
        self.ranges, self.k, self.seen = {}, {}, set()

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

    def arg(self, a):
        if isinstance(a, tuple) and a and a[0] == "struct":
            return "{" + " ".join(f"{n}={self.arg(v)}" for n, v in a[1]) + "}"
        if isinstance(a, int) and a >= 4096:
            for base, size in self.ranges.items():
                if base <= a < base + max(size, 1):
                    k = self.k.setdefault(base, len(self.k))
                    return f"buf{k}+{a - base}"
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
                s = args[-1] or 0   # (every launch takes the stream last; the ones of this process in order of appearance)
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
        bad = [k for k in a if k not in b or not torch.equal(a[k], b[k])] + [k for k in b if k not in a]
        print(f"{len(a)} inference outputs, {len(bad)} differ", *bad, sep="\n  ")
        sys.exit(1 if bad else 0)
    outs = {}
    with open(sys.argv[1], "w") as f:
        listing(f, outs)
    if len(sys.argv) > 2:
        torch.save(outs, sys.argv[2])
