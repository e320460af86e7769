#!/usr/bin/env python3
"""Generate tests/golden/paper_init_seed3.npz by running the *reference* in this container: the state_dict of the reference's
UNetModel on the paper 1-D configuration right after ``torch.manual_seed(3)``, as one fingerprint per tensor (the tensors
themselves are 62 MB).  tests/test_host.py::test_same_seed_same_weights_as_reference holds tqdne_amd's UNetModel to it.

  keys     parameter / buffer names in state_dict order
  sha256   per tensor: sha256 over dtype, shape and the raw bytes (tensor_fingerprint)
  head     per tensor: its first 8 entries as float64 (NaN-padded), to show where a mismatch starts

Run:  python tools/make_init_golden.py      (needs the reference checkout of make_goldens.REF; CPU only)
"""
import hashlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import make_goldens as mg  # noqa: E402

SEED = 3
HEAD = 8


def tensor_fingerprint(t: torch.Tensor) -> str:
    t = t.detach().cpu().contiguous()
    h = hashlib.sha256(f"{t.dtype}{tuple(t.shape)}".encode())
    h.update(t.numpy().tobytes())
    return h.hexdigest()


def tensor_head(t: torch.Tensor) -> np.ndarray:
    v = np.full(HEAD, np.nan)
    f = t.detach().cpu().reshape(-1)[:HEAD].double().numpy()
    v[:len(f)] = f
    return v


def main():
    sys.path.insert(0, mg.REF)
    from tqdne.unet import UNetModel as Ref
    from tqdne_amd import paper_1d_unet_config

    torch.manual_seed(SEED)
    sd = Ref(**paper_1d_unet_config()).state_dict()
    keys = list(sd)
    np.savez_compressed(os.path.join(mg.OUT, "paper_init_seed3.npz"), keys=np.array(keys),
                        sha256=np.array([tensor_fingerprint(sd[k]) for k in keys]),
                        head=np.stack([tensor_head(sd[k]) for k in keys]))
    print(f"{len(keys)} tensors written")


if __name__ == "__main__":
    main()
