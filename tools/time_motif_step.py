#!/usr/bin/env python3
"""Step time of the tree-only model 'prop' (PropertyVAE, forward + backward) at the shipped-config shape of the
prop_lstm_cfg_s62 fixture (LSTM, H = embed = 250, latent 24, depthT 20, diterT 1, B = 20), in the decoder's three
forms: the level through the tree-level driver (default), op by op (``_dev.TREE_DRIVER = False``) and the reference's step
loop (``_dev.DECODER_BATCHED = False``).  Prints one JSON line per form.

    python tools/time_motif_step.py [--steps 20] [--warmup 5] [--form driver|opbyop|stepwise|all]

Launches per step: the difference of two ``rocprofv3 --kernel-trace`` runs with ``--steps 3`` and ``--steps 1`` (same
``--warmup``), divided by two (model set-up and warm-up cancel)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

from motif_fixtures import MotifGolden  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--form", default="all", choices=["driver", "opbyop", "stepwise", "all"])
    a = ap.parse_args()
    from ggpm_amd import _dev
    g = MotifGolden("prop_lstm_cfg_s62")
    tensors, sch, orders, homos, lumos = g.batch()
    for form in (["driver", "opbyop", "stepwise"] if a.form == "all" else [a.form]):
        _dev.DECODER_BATCHED = form != "stepwise"
        _dev.TREE_DRIVER = form == "driver"
        model = g.model().cuda()
        times = []
        for i in range(a.warmup + a.steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            model.zero_grad(set_to_none=True)
            loss, _ = model(None, None, tensors, orders, homos, lumos, beta=g.beta, perturb_z=False, schedule=sch)
            loss.backward()
            torch.cuda.synchronize()
            if i >= a.warmup:
                times.append(time.perf_counter() - t0)
        times.sort()
        print(json.dumps({"model": "prop", "form": form, "B": g.B, "H": g.H, "steps": len(times),
                          "median_ms": 1e3 * times[len(times) // 2] if times else None,
                          "min_ms": 1e3 * times[0] if times else None}), flush=True)


if __name__ == "__main__":
    main()
