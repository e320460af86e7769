#!/usr/bin/env python3
"""Generate tests/golden/duration.npz with the reference's own functions of scripts/seismo_evaluations/arias_intensity_duration.ipynb.
The notebook is read as JSON and the one cell that defines ``calculate_arias_intensity`` (with ``compute_time_derivative``,
``calculate_resultant_horizontal`` and ``calculate_signal_duration``) is executed in a namespace that holds ``np`` and scipy's
``cumulative_trapezoid``; nothing of it is written anywhere.  The four functions are applied to seeded float32 waveforms as the
notebook's loop applies them.   Run: python tools/make_duration_goldens.py"""
import json
import os
import sys

import numpy as np
from scipy.integrate import cumulative_trapezoid

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import make_goldens as mg  # noqa: E402
import _duration_ref as DR  # noqa: E402

NOTEBOOK = os.path.join(mg.REF, "scripts", "seismo_evaluations", "arias_intensity_duration.ipynb")
SIZES = ((257, 3), (1000, 3), (4064, 2))   # (T, pairs)
PERCENTS = ((5, 95), (20, 75))


def reference_functions():
    cells = [c for c in json.load(open(NOTEBOOK))["cells"] if c["cell_type"] == "code" and "def calculate_arias_intensity" in "".join(c["source"])]
    assert len(cells) == 1
    ns = {"np": np, "cumulative_trapezoid": cumulative_trapezoid}
    exec("".join(cells[0]["source"]), ns)
    return ns


def main():
    ref = reference_functions()
    fx = {}
    for T, n in SIZES:
        x, y = DR.make_pairs(n, T, seed=11)
        w = np.stack([x, y], axis=1)                                   # (n, 2, T): channel 0 = NS, channel 1 = EW
        time = np.linspace(0, 0.01 * T, T)                             # the notebook's time axis
        acc = ref["calculate_resultant_horizontal"](w[:, 1], w[:, 0])  # float32
        fx[f"w{T}"], fx[f"time{T}"] = w, time
        if T == 257:
            fx[f"resultant{T}"] = acc
            fx[f"gradient{T}"] = ref["compute_time_derivative"](w)     # float32
            fx[f"gradient50_{T}"] = ref["compute_time_derivative"](w, sampling_rate=50)
        for tag, rows in (("raw", acc), ("norm", np.stack([a / max(abs(a)) for a in acc]))):
            Ia, cum, dur, idx = [], [], [], []
            for a in rows:
                ia, c = ref["calculate_arias_intensity"](time, a)
                Ia.append(ia), cum.append(c)
                d = [ref["calculate_signal_duration"](time, c, ia, lower_percent=lo, upper_percent=hi) for lo, hi in PERCENTS]
                dur.append(d)
                idx.append([[int(np.flatnonzero(time == t)[0]) for t in one[:2]] for one in d])
            fx[f"{tag}_Ia{T}"] = np.array(Ia)                          # (n,)
            fx[f"{tag}_dur{T}"] = np.array(dur)                        # (n, 2, 3): per percent pair t_start, t_end, duration
            fx[f"{tag}_idx{T}"] = np.array(idx, np.int32)              # (n, 2, 2)
            if T < 4064 and tag == "raw":
                fx[f"{tag}_cum{T}"] = np.array(cum)                    # (n, T) float64
        # one component, as the notebook's second figure uses it
        ia, c = ref["calculate_arias_intensity"](time, w[0, 0])
        fx[f"single_Ia{T}"] = np.array(ia)
        fx[f"single_dur{T}"] = np.array(ref["calculate_signal_duration"](time, c, ia, lower_percent=5, upper_percent=95))
        fracs = sorted({p / 100 for pair in PERCENTS for p in pair})
        print(T, "crossing margin of the float64 restatement, resultant:", DR.crossing_margin(DR.cumulative(x, y, time[1]), fracs),
              "single:", DR.crossing_margin(DR.cumulative(x[:1], None, time[1]), [0.05, 0.95]))
    fx["percents"] = np.array(PERCENTS)
    path = os.path.join(mg.OUT, "duration.npz")
    np.savez_compressed(path, **fx)
    print({k: (v.shape, str(v.dtype)) for k, v in fx.items()}, os.path.getsize(path))


if __name__ == "__main__":
    main()
