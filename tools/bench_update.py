#!/usr/bin/env python3
"""Developer tool (GPU box): the Momentum + re-pack pass (rsu_update_table_run) alone: us per call and GB/s at 24 B per parameter, for the c2 and the c3
network. `adam`: the Adam pass (rsu_update_table_run_adam, 32 B per packed weight) next to the Momentum pass of the same run, each timed on its own
net, with the library hash. usage: bench_update.py [adam] [c2] [c3]"""
import hashlib, os, sys, time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from road_segmentation_unet_amd import _lib
from road_segmentation_unet_amd.unet import UNet


def median_us(step):
    for _ in range(5): step()
    torch.cuda.synchronize()
    ts = []
    for _ in range(30):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); step(); b.record(); b.synchronize(); ts.append(a.elapsed_time(b) * 1e3)
    ts.sort()
    return ts[len(ts) // 2]


args = sys.argv[1:]
adam = "adam" in args
wls = [a for a in args if a != "adam"] or ["c2", "c3"]
if adam:
    print("librsu_hip.so sha16 %s" % hashlib.sha256(open(_lib.LIB_PATH, "rb").read()).hexdigest()[:16])
for wl in wls:
    L, dil, B = (5, False, 4) if wl == "c2" else (6, True, 1)
    m = UNet(L, 64, dil, B, 388, training=True)
    m.flat_g.normal_(0, 1e-3)
    us = median_us(lambda: m.apply_momentum(0.0, 0.9))
    print("%s: %d live parameters, update %.1f us (median of 30) = %.2f TB/s at 24 B per parameter" % (wl, m.n_live, us, m.n_live * 24 / us / 1e6))
    n_live = m.n_live
    del m
    if adam:
        a = UNet(L, 64, dil, B, 388, training=True, optimizer="adam")
        a.flat_g.normal_(0, 1e-3)
        ua = median_us(lambda: a.apply_adam(0.0))
        print("%s: %d live parameters, Adam update %.1f us (median of 30) = %.2f TB/s at 32 B per parameter; %.3f x the Momentum pass (32/24 = 1.333)"
              % (wl, n_live, ua, n_live * 32 / ua / 1e6, ua / us))
        del a
