"""Cost of the classifier head on the HIP path, at the reference's classifier encoder (experiments/train_classifier.py:70-82) in its
1-D form: dims=1, conv_kernel_size=3, 3 x 4096 waveforms, B = 128, 36 classes.

    python tools/bench_classifier.py [--batch B] [--length T] [--rounds R] [--json OUT.json]

HIP events around launches issued back to back, medians over the rounds:
  embed       ``classifier.embed(x)`` in eval mode (encoder plan + tq_classifier_head_fwd): waveforms / s
  encoder     the encoder plan alone, forward (channels-last output) and forward + backward (training mode, dropout 0.1)
  head        the three head launches: tq_classifier_head_fwd, tq_cross_entropy, tq_classifier_head_bwd (itself three kernels)
  torch head  the same head written as torch ops on the same channels-last tensor: ``mean`` + ``nn.Sequential`` + ``nn.Linear`` +
              ``F.cross_entropy`` + autograd down to d loss / d h (B, T', C)
  layout flip the (B, T', C) -> (B, C, T') copy the NCW route would add in front of a torch head, and its mirror in the backward"""

import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ENCODER = dict(in_channels=3, model_channels=64, channel_mult=(1, 2, 4, 4), out_channels=256, num_res_blocks=2,
               attention_resolutions=(8,), dims=1, conv_kernel_size=3, num_heads=4, dropout=0.1, flash_attention=False)


def event_ms(fn, n=5):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--length", type=int, default=4096)
    ap.add_argument("--classes", type=int, default=36)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()

    from tqdne_amd import LithningClassifier, _lib, rng
    from tqdne_amd._lib import _p, check
    from tqdne_amd.autoencoder import _seq_engine

    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    B, K = a.batch, a.classes
    clf = LithningClassifier(ENCODER, K, nn.CrossEntropyLoss(weight=0.5 + torch.rand(K)), [],
                             {"learning_rate": 1e-4, "max_steps": 1000, "eta_min": 0.0})
    with torch.no_grad():
        for p in clf.parameters():
            if torch.count_nonzero(p) == 0:
                p.normal_(0, 0.02)
    clf = clf.to(dev)
    g = torch.Generator().manual_seed(1)
    x = (0.5 * torch.randn(B, 3, a.length, generator=g)).to(dev)
    y = torch.randint(0, K, (B,), generator=g).to(dev)
    rng.seed_rank(0, 0)
    lib = _lib.load()
    stream = torch.cuda.current_stream(dev).cuda_stream

    clf.eval()
    with torch.no_grad():
        clf.embed(x)
    clf.train()
    clf.step_and_backward({"signal": x, "label": y})   # (builds both plans and the head's buffers)
    eng = _seq_engine(clf.encoder, x)
    bufs = next(iter(clf._head_bufs.values()))
    h = eng.head_btc.buf
    _, Tp, C = h.shape
    W1, b1, W2, b2, W3, b3 = clf._head_params()
    gr = [torch.empty_like(p) for p in (W3, b3, W2, b2, W1, b1)]
    dh = eng.backward_plan().dout_btc

    def embed():
        with torch.no_grad():
            clf.embed(x)

    def enc_fwd():
        eng.forward(x, train=True, dropout_seed=1, channels_last=True)

    def enc_fwd_bwd():
        eng.forward(x, train=True, dropout_seed=1, channels_last=True)
        eng.backward(None, clone=False)

    def head_fwd():
        check(lib.tq_classifier_head_fwd(_p(h), _p(W1), _p(b1), _p(W2), _p(b2), _p(W3), _p(b3), _p(bufs["pooled"]), _p(bufs["a1"]),
                                         _p(bufs["emb"]), _p(bufs["logits"]), B, Tp, C, K, stream))

    def head_ce():
        check(lib.tq_cross_entropy(_p(bufs["logits"]), _p(y), _p(clf.loss.weight), -100, _p(bufs["loss"]), _p(bufs["dlogits"]), B, K, stream))

    def head_bwd():
        check(lib.tq_classifier_head_bwd(_p(bufs["dlogits"]), _p(bufs["pooled"]), _p(bufs["a1"]), _p(bufs["emb"]), _p(W1), _p(W2), _p(W3),
                                         *[_p(t) for t in gr], _p(dh), _p(bufs["ws"]), bufs["nws"], B, Tp, C, K, stream))

    def head_all():
        head_fwd(), head_ce(), head_bwd()

    hl = h.clone().requires_grad_(True)

    def torch_head():
        hl.grad = None
        clf.zero_grad(set_to_none=True)
        logits = clf.output_layer(clf.output_MLP(hl.mean(1)))
        F.cross_entropy(logits, y, clf.loss.weight).backward()

    nct = torch.empty(B, C, Tp, device=dev)

    def flips():
        nct.copy_(h.permute(0, 2, 1))
        dh.copy_(nct.permute(0, 2, 1))

    fns = dict(embed=embed, encoder_fwd=enc_fwd, encoder_fwd_bwd=enc_fwd_bwd, head_fwd=head_fwd, cross_entropy=head_ce, head_bwd=head_bwd,
               head=head_all, torch_head=torch_head, layout_flips=flips)
    for fn in fns.values():
        fn()
    rows = {k: [] for k in fns}
    for r in range(a.rounds):
        for k, fn in fns.items():
            rows[k].append(event_ms(fn, 3 if k.startswith(("embed", "encoder")) else 20))
        print(f"round {r}: " + ", ".join(f"{k} {v[-1]:.4f}" for k, v in rows.items()) + " ms", flush=True)
    ms = {k: statistics.median(v) for k, v in rows.items()}
    res = dict(device=torch.cuda.get_device_name(0), batch=B, length=a.length, pooled_length=Tp, channels=C, classes=K, rounds=a.rounds,
               ms=ms, embed_waveforms_per_s=B / ms["embed"] * 1e3, head_share_of_step=ms["head"] / (ms["encoder_fwd_bwd"] + ms["head"]))
    print(f"classifier at B = {B}, 3 x {a.length} (T' = {Tp}, C = {C}, K = {K}) on {res['device']}, medians of {a.rounds}:\n"
          f"  embed() {ms['embed']:.2f} ms = {res['embed_waveforms_per_s']:.0f} waveforms/s\n"
          f"  encoder forward {ms['encoder_fwd']:.2f} ms, forward + backward {ms['encoder_fwd_bwd']:.2f} ms\n"
          f"  head: forward {1e3 * ms['head_fwd']:.1f} us, cross-entropy {1e3 * ms['cross_entropy']:.1f} us, backward "
          f"{1e3 * ms['head_bwd']:.1f} us; together {1e3 * ms['head']:.1f} us = {100 * res['head_share_of_step']:.3f} % of the step\n"
          f"  the same head as torch ops (forward + loss + autograd): {1e3 * ms['torch_head']:.1f} us; the two layout flips of the NCW "
          f"route: {1e3 * ms['layout_flips']:.1f} us")
    print("RESULT " + json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
