#!/usr/bin/env python3
"""Headline benchmark: 388x388 patches/s of the fused forward + backward + Momentum step (BASELINE.json metric).

    python bench.py --gpus N --steps K --warmup W [--full] [--dump-outputs DIR]
    (N > 1: python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 ... bench.py --gpus N ...)

A plain run does what the headline figure needs and nothing else: set up (explicit tile-shape tuning pass, untimed priming), W
warm-up steps, K timed steps, the outputs of the last timed step written to DIR (--dump-outputs), one JSON line. The model state is
reset to its seeded initial value behind the priming, so the last timed step is step W + K from the same weights on the same
inputs in every run with the same arguments: two builds can be compared output for output. Everything else below (`sustained`,
the instrumented roofline passes, the exchange proof for N > 1, the CPU baselines) runs behind --full only.

Workload = BASELINE.json configs[1]: num_layers=5 root_size=64 patch_size=388 (input 572), bf16 storage / fp32
accumulate, 4 patches per GPU (weak scaling: the global batch is 4*N), synthetic data of SURVEY.md section 8(d):
X ~ U[0,1), labels ~ Bernoulli(0.2), Glorot-uniform weights, lr 0.01, momentum 0.9, dropout_keep 1.0. A step is
session.run([train, loss, predictions]) of the reference (tf_aerial_images.py:241-244): forward, loss, full backward,
gradient all-reduce over RCCL when N > 1, Momentum update of every live variable and the bf16 re-pack of the weights.
The weight-gradient launches of a step run on a second HIP stream beside the backward-data launches (RSU_WGRAD_STREAM=0: one stream).
Inputs are resident in HBM before the timed region (the reference feeds host numpy arrays; the PCIe-inclusive figure is
discussed in DESIGN.md and is never `value`).

Besides the contract line the JSON carries (plain run: `roofline` holds only `whole_step_frac`, which needs no run of its own)
  roofline     : the 3x3-conv MFMA kernels (forward, backward-data, backward-weight): algorithmic FLOPs
                 (2*B*Ho*Wo*Cout*Cin*9 per launch) / the CHIP TIME of those launches in the very schedule `value`
                 is timed on, measured with HIP events on each launch's own stream in an instrumented pass right behind the
                 timed region. Chip time of a launch = its duration x the share of the 256 CUs it plans for (its `ncu`
                 argument): forward launches have the chip to themselves (share 1), in the backward pass a backward-data and a
                 weight-gradient kernel run side by side on 128 CUs each (share 1/2 each). peak = 2.5 PFLOP/s dense bf16
                 MFMA (/opt/skills/guides/MI355X_MICROARCH.md). Two serialised single-stream passes (every kernel alone on
                 the chip) follow for comparison: `frac_serial_per_layer` (one weight-gradient launch per layer, rounds 1-2's
                 definition) and `frac_single_stream_grouped` (the single-stream product schedule with grouped weight
                 gradients, round 3's headline). `frac` is an upper bound of the kernels' efficiency (a launch is billed the CUs
                 it plans for); `frac_busy_union` is the lower bound (the whole chip billed whenever any 3x3-conv launch runs),
                 `whole_step_frac` the figure over the whole timed step. `traffic` comes from a committed PMC run and is null unless that file was
                 measured with this very build of librsu_hip.so (sha-256 match).
  cpu_baseline : the CPU oracle (oracle/unet_oracle.c, kind "port"; TensorFlow 1.4 cannot be installed) timed on the
                 host cores on a bounded sample of the same network, rank 0 / N=1 only.
  cpu_baseline_torch : the same step in stock PyTorch-CPU float32 (oneDNN, oracle/torch_ref.py; kind "stand-in").
  sustained    : the same loop run for >= 2 s behind the timed region (clocks and power at steady state).

--dump-outputs DIR writes what a caller of the step receives from the last timed step (rank 0): loss.npy (float64, the global mean
loss), predictions.npy (float32 [B, P, P] road probabilities of rank 0's patches), weights_sample.npy and momentum_sample.npy
(float32: the updated variables and their Momentum slots, every live variable in name order, all of it up to 16384 values per
variable and a fixed seeded sample of that many beyond).

--workload c4 switches to BASELINE.json configs[3]'s per-GPU share (num_layers=6, 4 patches per GPU) for scaling runs of the
data-parallel configuration; --workload c3 to configs[2] (num_layers=6, --dilated_layers, ONE patch per step: the reference's
final model as it trains it, README.md:49-66); the default (c2) is the configuration the metric is quoted on.

`python bench.py --gpus N` with N > 1 and no WORLD_SIZE in the environment starts its own ranks: it runs
`python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port <free> bench.py ...` as a CHILD
process before anything touches the GPU, relays the ranks' output and exits with the child's return code.
"""
import hashlib
import argparse
import ctypes
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from road_segmentation_unet_amd._lib import call, lib  # noqa: E402
from road_segmentation_unet_amd.dist import GradBucketer, tune_overlap  # noqa: E402
from road_segmentation_unet_amd.unet import UNet, input_size_needed  # noqa: E402

MFMA_BF16_PEAK_TFLOPS = 2500.0  # dense, MI355X_MICROARCH.md "Peak BF16/FP16 MFMA"


def run_step(m, bucketer, lr, mu):
    m.forward_device()
    if bucketer is not None:
        bucketer.reset()
    # single device: the Momentum step + re-pack of the conv kernels rides on their weight-gradient launches (UNet.backward_device)
    m.backward_device(m._inv_count, update=(lr, mu) if bucketer is None else None)
    if bucketer is not None:
        bucketer.finish()
    m.apply_momentum(lr, mu)


def physical_cores():
    try:
        import psutil
        return psutil.cpu_count(logical=False) or os.cpu_count()
    except Exception:
        return os.cpu_count()


def cpu_baseline(L, root, sample_P, threads, repeats=2):
    """Oracle (C port of the reference's graph) on the host cores: fwd+bwd+Momentum steps on a bounded sample -- one untimed
    warm-up step on a small patch (OpenMP thread start, page faults of the library), then the best of `repeats` timed steps.
    The OpenMP team is set to `threads` (the physical cores: the same count the PyTorch leg uses)."""
    from oracle import unet_oracle as U
    U.lib()
    try:
        ctypes.CDLL("libgomp.so.1").omp_set_num_threads(int(threads))
    except OSError:
        threads = os.cpu_count()
    rng = np.random.RandomState(2017)

    def sample(P):
        S = U.input_size_needed(P, L)
        return rng.rand(1, S, S, 3).astype(np.float32), (rng.rand(1, P, P) < 0.2).astype(np.int64), S
    params = U.init_params(L, root, False, seed=2018)
    acc = {k: np.zeros_like(v) for k, v in params.items()}
    Xw, lw, _ = sample(36)
    U.train_step(params, acc, Xw, lw, L, root, False)
    X, labels, S = sample(sample_P)
    best = float("inf")
    for _ in range(repeats):
        t0 = time.time()
        U.train_step(params, acc, X, labels, L, root, False)
        best = min(best, time.time() - t0)
    return best, S, threads


def net_flops(L, root, dilated, P, B):
    """algorithmic FLOPs of one fwd+bwd step: (total, 3x3 convs) following BASELINE.md section 2 (dead ops excluded)."""
    S = input_size_needed(P, L)
    tot = conv3 = 0.0
    h, nf, cin = S, root, 3
    tot += 2 * 2.0 * B * S * S * 3 * 3  # color adjust: fwd + bwd-weight only
    enc = []
    for i in range(L):
        last = i == L - 1
        f1 = 2.0 * B * (h - 2) ** 2 * nf * cin * 9
        f2 = 2.0 * B * (h - 4) ** 2 * nf * nf * 9
        mult1 = 2 if i == 0 else 3  # no bwd-data into the 3-channel input
        conv3 += mult1 * f1 + 3 * f2
        if dilated and not last:
            d1 = 2.0 * B * (h - 4) ** 2 * nf * cin * 9
            d2 = 2.0 * B * (h - 8) ** 2 * nf * nf * 9
            conv3 += mult1 * d1 + 3 * d2
        enc.append((h - 4, nf))
        if not last:
            h = (h - 4) // 2
            cin, nf = nf, nf * 2
    h = h - 4
    up = 0.0
    for i in range(L - 1):
        nf //= 2
        up += 3 * 2.0 * B * h * h * 4 * nf * (2 * nf)
        h *= 2
        ccat = (3 if dilated else 2) * nf
        conv3 += 3 * (2.0 * B * (h - 2) ** 2 * nf * ccat * 9 + 2.0 * B * (h - 4) ** 2 * nf * nf * 9)
        h -= 4
    head = 3 * 2.0 * B * P * P * root * 2
    tot += conv3 + up + head
    return tot, conv3


DUMP_PER_VARIABLE = 16384   # values of one variable written by --dump-outputs (all of them when it has no more)


def sample_values(a, k, seed):
    """a flattened, all of it when it has at most k values, else the values at k fixed positions (ascending) drawn with `seed`"""
    a = np.asarray(a).reshape(-1)
    if a.size <= k:
        return a
    return a[np.sort(np.random.RandomState(seed).choice(a.size, k, replace=False))]


def dump_outputs(out_dir, loss, predictions, variables):
    """--dump-outputs: loss (float64), predictions (float32) and the sampled variables / Momentum slots (float32) as out_dir/<name>.npy.
    variables: [(name, weights, momentum)] of numpy arrays in a fixed order; each variable's sample positions are seeded by its index."""
    os.makedirs(out_dir, exist_ok=True)
    w = [sample_values(v, DUMP_PER_VARIABLE, 1000 + i) for i, (_, v, _) in enumerate(variables)]
    a = [sample_values(v, DUMP_PER_VARIABLE, 1000 + i) for i, (_, _, v) in enumerate(variables)]
    arrays = {"loss": np.asarray([loss], dtype=np.float64),
              "predictions": np.asarray(predictions, dtype=np.float32),
              "weights_sample": np.concatenate(w).astype(np.float32),
              "momentum_sample": np.concatenate(a).astype(np.float32)}
    total = sum(v.nbytes for v in arrays.values())
    assert total <= 64 << 20, "--dump-outputs would write %d bytes (> 64 MB)" % total
    for name, v in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), v)
    return arrays


def launch_ranks(nranks, script, script_args, timeout=None):
    """Start `script` under torch.distributed.run with `nranks` ranks on this node as a child process (never an exec: a process that
    has touched the GPU must not be replaced), relay its stdout / stderr and return its exit code. One rank per GPU over RCCL
    (RSU_BENCH_BACKEND=gloo: the ranks share whatever GPUs exist -- tests)."""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # dmabuf IPC only on this driver (RCCL, CUDA-tensor sharing)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nranks), "--master-addr", "127.0.0.1",
           "--master-port", str(port), script] + list(script_args)
    proc = subprocess.run(cmd, env=env, timeout=timeout)
    return proc.returncode


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--num_layers", type=int, default=5)
    ap.add_argument("--root_size", type=int, default=64)
    ap.add_argument("--patch_size", type=int, default=388)
    ap.add_argument("--batch_per_gpu", type=int, default=None, help="patches per GPU and step (default 4; 1 for --workload c3)")
    ap.add_argument("--dilated_layers", action="store_true")
    ap.add_argument("--no_cpu_baseline", action="store_true")
    ap.add_argument("--workload", default=os.environ.get("RSU_BENCH_WORKLOAD", "c2"), choices=["c2", "c3", "c4"],
                    help="c2: num_layers=5 (headline); c3: num_layers=6 dilated, one patch per step (the reference's final model); "
                         "c4: num_layers=6, the per-GPU share of the data-parallel configuration")
    ap.add_argument("--sustain_seconds", type=float, default=5.0, help="length of the extra steady-state loop (0: skip); 5 s: longer than the period of the driver's GPU-busy sampler (VERDICT r5 item 14)")
    ap.add_argument("--prime_seconds", type=float, default=1.0,
                    help="untimed steps run for this long in front of the W warm-up steps: clocks and power reach their steady state (0: skip)")
    ap.add_argument("--cpu_sample_patch", type=int, default=196)
    ap.add_argument("--full", action="store_true",
                    help="also run what the headline figure does not need: the sustained loop, the instrumented roofline passes, the exchange "
                         "proof (N > 1) and the CPU baselines")
    ap.add_argument("--dump-outputs", dest="dump_outputs", metavar="DIR", default=None,
                    help="write the outputs of the last timed step as DIR/<name>.npy (loss, predictions, sampled weights / Momentum slots)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # bare `bench.py --gpus N`: this process becomes the launcher of N ranks (nothing has touched the GPU yet)
        sys.exit(launch_ranks(args.gpus, os.path.abspath(__file__), sys.argv[1:]))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    # RSU_BENCH_BACKEND=gloo (tests only): the same multi-rank code path with the ranks sharing whatever GPUs exist -- RCCL
    # refuses two ranks on one device, and the GPU test box has one
    backend = os.environ.get("RSU_BENCH_BACKEND", "nccl")
    gpu_index = local_rank if backend == "nccl" else local_rank % max(1, torch.cuda.device_count())
    if args.gpus > 1 or world > 1:
        assert world == args.gpus, "launch with torch.distributed.run --nproc-per-node %d" % args.gpus
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        torch.cuda.set_device(gpu_index)
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", gpu_index))
        else:
            dist.init_process_group(backend)
    dev = "cuda:%d" % gpu_index
    torch.cuda.set_device(gpu_index)

    if args.workload == "c4":
        args.num_layers = 6
    if args.workload == "c3":
        args.num_layers, args.dilated_layers = 6, True
        if args.batch_per_gpu is None:
            args.batch_per_gpu = 1   # the reference trains this model at batch 1 (README.md:54)
    if args.batch_per_gpu is None:
        args.batch_per_gpu = 4
    L, root, P, B = args.num_layers, args.root_size, args.patch_size, args.batch_per_gpu
    lib_sha = hashlib.sha256(open(os.path.join(ROOT, "road_segmentation_unet_amd", "librsu_hip.so"), "rb").read()).hexdigest()[:16]
    tune_file = os.environ.get("RSU_AUTOTUNE_FILE")  # profile runs: re-use the tile shapes a previous run measured (no timing launches)
    tune_imported = False
    if tune_file and os.path.exists(tune_file):
        tj = json.load(open(tune_file))
        # the file carries the hash of the library that measured it: a table of another build is ignored (its shape ids may be gone)
        if isinstance(tj, dict) and tj.get("lib_sha16") == lib_sha:
            tab = tj["rows"]
            arr = (ctypes.c_int * len(tab))(*tab)
            taken = lib().rsu_autotune_import(arr, len(tab) // 17)
            tune_imported = taken == len(tab) // 17
            if not tune_imported:
                print("bench.py: %s: only %d of %d rows imported" % (tune_file, taken, len(tab) // 17), file=sys.stderr)
        else:
            print("bench.py: %s was measured with another build of librsu_hip.so: ignored" % tune_file, file=sys.stderr)
    S = input_size_needed(P, L)
    m = UNet(L, root, args.dilated_layers, B, P, device=dev, seed=2018, training=True)
    m._inv_count = 1.0 / (world * B * P * P)
    g = torch.Generator(device="cpu").manual_seed(2017 + rank)
    m.x.copy_(torch.rand((B, S, S, 3), generator=g))
    m.labels.copy_((torch.rand((B, P, P), generator=g) < 0.2).to(torch.int64))
    bucketer = None
    if world > 1:
        bucketer = GradBucketer(m.flat_g, m.n_live)
        bucketer.extra_streams = list(m.wstreams)
        m.on_grads = bucketer.ready
    lr, mu = 0.01, 0.9
    # developer switch (tools/dp_budget.sh): the CU budget a data-parallel run would give the backward launches (dist.tune_overlap's candidates),
    # on one GPU, with the update left behind the pass as under an exchange -- what does leaving CUs to RCCL's channel workgroups cost?
    if os.environ.get("RSU_BENCH_BWD_BUDGET"):
        m.backward_cu_budget = int(os.environ["RSU_BENCH_BWD_BUDGET"])

    # the explicit tile-shape tuning pass (UNet.tune: one untimed forward + backward in RSU_TUNE_MEASURE mode; the launches of the
    # timed region only look shapes up), skipped when a table measured by this very build was imported; then one untimed priming step
    if not tune_imported:
        m.tune()
    # the seeded initial state: restored behind the untimed steps below, whose number depends on timing, so that the warm-up and timed
    # steps start from the same weights in every run
    init_state = (m.flat_w.clone(), m.flat_acc.clone(), m.global_step)
    run_step(m, bucketer, lr, mu)
    dp_tune = None
    if bucketer is not None and "RSU_DP_OVERLAP" not in os.environ:
        # untimed: measure both gradient-exchange schedules on this node and keep the faster one (dist.tune_overlap)
        def set_budget(n):
            m.backward_cu_budget = n
            if not tune_imported:
                m.ensure_tuned()
        dp_tune = tune_overlap(bucketer, lambda: run_step(m, bucketer, lr, mu), set_cu_budget=set_budget)
    # priming (untimed): the timed region is ~0.1 s long, the chip needs about a second of this load to settle its clocks (the 2-s
    # `sustained` loop behind the timed region read ~1 % above it without this); every rank runs the same number of steps
    if args.prime_seconds > 0:
        torch.cuda.synchronize()
        tp = time.perf_counter()
        for _ in range(5):
            run_step(m, bucketer, lr, mu)
        torch.cuda.synchronize()
        per = (time.perf_counter() - tp) / 5
        nprime = int(args.prime_seconds / max(per, 1e-4))
        if world > 1:
            tn = torch.tensor([nprime], dtype=torch.int64, device=dev)
            dist.all_reduce(tn, op=dist.ReduceOp.MIN)
            nprime = int(tn.item())
        for _ in range(nprime):
            run_step(m, bucketer, lr, mu)
    torch.cuda.synchronize()
    m.flat_w.copy_(init_state[0])
    m.flat_acc.copy_(init_state[1])
    m.global_step = init_state[2]
    m.repack()
    del init_state
    for _ in range(args.warmup):
        run_step(m, bucketer, lr, mu)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        run_step(m, bucketer, lr, mu)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([dt], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    loss_t = m.loss_sum.clone()
    if world > 1:
        dist.all_reduce(loss_t)  # every rank holds the sum over ITS pixels; _inv_count is 1 / global pixel count
    loss = float(loss_t.item()) * m._inv_count
    if args.dump_outputs and rank == 0:
        live = [n for n in m.names if m._slices[n][0] < m.n_live]
        dump_outputs(args.dump_outputs, loss, m.prob.cpu().numpy(),
                     [(n, m.w[n].cpu().numpy(), m.acc[n].cpu().numpy()) for n in live])
    # ---- everything below up to the result line runs with --full only
    # ---- sustained figure: the same loop for >= 2 s (the timed region above is ~0.1 s: too short for clocks / power to settle)
    sustained = None
    if args.full and args.sustain_seconds > 0:
        nsus = max(args.steps, int(args.sustain_seconds / (dt / args.steps)) + 1)
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        ts = time.perf_counter()
        for _ in range(nsus):
            run_step(m, bucketer, lr, mu)
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        dsus = time.perf_counter() - ts
        if world > 1:
            t = torch.tensor([dsus], dtype=torch.float64, device=dev)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            dsus = float(t.item())
        sustained = {"value": world * B * nsus / dsus, "unit": "patches/s", "steps": nsus, "seconds": dsus, "ms_per_step": dsus / nsus * 1e3}
    # ---- proof of exchange (untimed, N > 1): one backward pass WITHOUT the exchange gives every rank's own gradient checksum; their sum
    # over the ranks must equal the checksum of the all-reduced buffer, which must be identical on every rank
    dp_proof = None
    if args.full and bucketer is not None:
        on_grads, m.on_grads = m.on_grads, None
        m.forward_device()
        m.backward_device(m._inv_count)
        m.on_grads = on_grads
        torch.cuda.synchronize()
        local = m.flat_g[:m.n_live].double().sum().reshape(1)
        sum_local = local.clone()
        dist.all_reduce(sum_local)
        dist.all_reduce(m.flat_g[:m.n_live])
        red = m.flat_g[:m.n_live].double().sum().reshape(1)
        rmin, rmax = red.clone(), red.clone()
        dist.all_reduce(rmin, op=dist.ReduceOp.MIN)
        dist.all_reduce(rmax, op=dist.ReduceOp.MAX)
        try:
            ver = ".".join(str(v) for v in torch.cuda.nccl.version()) if backend == "nccl" else None
        except Exception:
            ver = None
        dp_proof = {"backend": dist.get_backend(), "rccl_version": ver, "world_size": dist.get_world_size(),
                    "payload_MB": m.n_live * 4 / 1e6, "checksum_rank0_local": float(local.item()),
                    "checksum_sum_of_ranks": float(sum_local.item()), "checksum_allreduced_min_over_ranks": float(rmin.item()),
                    "checksum_allreduced_max_over_ranks": float(rmax.item())}
    tot_fl, conv3_fl = net_flops(L, root, args.dilated_layers, P, B)
    # (plain run: the only roofline figure that needs no run of its own)
    roofline = {"bound": "mfma", "peak": MFMA_BF16_PEAK_TFLOPS, "unit": "TFLOP/s",
                "whole_step_frac": conv3_fl * world / (dt / args.steps) / 1e12 / (MFMA_BF16_PEAK_TFLOPS * world)}
    if args.full:
        # ---- instrumented passes (HIP events on the launch's own stream around every 3x3-conv MFMA launch)
        nprof = 3

        def instrumented(label):
            """nprof steps with events around every 3x3-conv launch -> (achieved TFLOP/s over chip time, by_kernel, launches, chip seconds)"""
            run_step(m, bucketer, lr, mu)   # untimed
            torch.cuda.synchronize()
            m.prof = []
            for _ in range(nprof):
                run_step(m, bucketer, lr, mu)
            torch.cuda.synchronize()
            agg = {}
            spans = []
            ref = m.prof[0][2] if m.prof else None
            for tag, fl, e0, e1, share in m.prof:
                a = agg.setdefault(tag, [0.0, 0.0, 0, 0.0])
                dur = e0.elapsed_time(e1) * 1e-3
                a[0] += fl
                a[1] += dur * share      # chip time: a launch planned for half of the CUs runs beside another one
                a[2] += 1
                a[3] += dur
                t0_ = ref.elapsed_time(e0) * 1e-3
                spans.append((t0_, t0_ + dur))
            m.prof = None
            # union of the launches' busy intervals over both streams: the time during which AT LEAST ONE 3x3-conv launch held (part of) the
            # chip. FLOPs over it bills the whole chip for every such moment -- a LOWER bound of the kernels' efficiency, where `achieved`
            # (duration x planned CU share) is an upper bound whenever the two backward streams do not overlap perfectly
            spans.sort()
            union, cur0, cur1 = 0.0, None, None
            for a0, a1 in spans:
                if cur1 is None or a0 > cur1:
                    if cur1 is not None:
                        union += cur1 - cur0
                    cur0, cur1 = a0, a1
                else:
                    cur1 = max(cur1, a1)
            if cur1 is not None:
                union += cur1 - cur0
            fl = sum(a[0] for a in agg.values())
            t = sum(a[1] for a in agg.values())
            n = sum(a[2] for a in agg.values())
            by = {k: {"tflops": v[0] / v[1] / 1e12, "chip_ms_per_step": v[1] / nprof * 1e3, "wall_ms_per_step": v[3] / nprof * 1e3,
                      "launches": v[2] // nprof} for k, v in agg.items()}
            return {"achieved": fl / t / 1e12 if t > 0 else 0.0, "by_kernel": by, "launches": n, "chip_s": t, "flops": fl, "label": label,
                    "busy_union_s": union}

        # (1) the timed schedule itself: two streams in the backward pass, every launch with the CU share it has there. The conv launches of a
        # step cannot hold the chip for longer than the step lasts: a pass whose chip time exceeds the timed step by more than 15 % is not a
        # measurement of that schedule (seen once in ~30 runs on the test pool: both backward queues reported ~6x their usual kernel durations
        # for one pass, profiles/r04/bench_odd_pass.json) and is repeated, at most twice.
        attempts = 0
        while True:
            attempts += 1
            prof_timed = instrumented("timed schedule")
            plausible = prof_timed["chip_s"] / nprof <= 1.15 * dt / args.steps
            if world > 1:
                # every rank repeats the pass or none does: its steps hold collectives (round 4: decided per rank, one rank ran a pass more than
                # its peer and the run ended in "connection reset by peer" -- two of eight two-rank runs on a shared GPU)
                ok = torch.tensor([1 if plausible else 0], dtype=torch.int32, device=dev if backend == "nccl" else "cpu")
                dist.all_reduce(ok, op=dist.ReduceOp.MIN)
                plausible = bool(ok.item())
            if plausible or attempts >= 3:
                break
        # (2), (3) serialised single-stream passes, every launch alone on the chip: one weight-gradient launch per layer (rounds 1-2's
        # figure), then the single-stream product schedule with grouped weight gradients (round 3's headline figure)
        wstreams, m.wstreams = m.wstreams, []
        if not tune_imported:
            m.tune()                    # on one stream the backward launches plan for the whole chip: shapes not measured yet
        wg_env = os.environ.get("RSU_WG_GROUP")
        os.environ["RSU_WG_GROUP"] = "0"
        prof_serial = instrumented("single stream, one weight-gradient launch per layer")
        if wg_env is None:
            del os.environ["RSU_WG_GROUP"]
        else:
            os.environ["RSU_WG_GROUP"] = wg_env
        prof_grouped = instrumented("single stream, grouped weight gradients") if wstreams else prof_serial
        m.wstreams = wstreams
        # (the table of measured tile shapes: saved behind BOTH schedules -- they plan the backward launches for different CU budgets)
        if tune_file and rank == 0 and not os.path.exists(tune_file):
            cap = lib().rsu_autotune_entries()
            arr = (ctypes.c_int * (17 * max(1, cap)))()
            n = lib().rsu_autotune_export(arr, cap)
            json.dump({"lib_sha16": lib_sha, "rows": list(arr[:17 * n])}, open(tune_file, "w"))

        two_streams = bool(wstreams)
        achieved = prof_timed["achieved"]
        n_launch = prof_timed["launches"]
        conv_t = prof_timed["chip_s"]
        conv_fl = prof_timed["flops"]
        # HBM-side bytes per conv launch: PMC counters cannot be read from inside this process; the figure is the one measured with
        # tools/pmc_traffic.sh on this same workload and committed under profiles/rNN/traffic.json (null for any other workload)
        traffic, traffic_source = None, None
        try:
            import glob
            for cand in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*", "traffic.json")), reverse=True):
                tj = json.load(open(cand))
                if tj.get("lib_sha16") == lib_sha and (L, root, P, B, args.dilated_layers) == (5, 64, 388, 4, False):
                    traffic = tj["kernels"]["conv3x3 all"]["hbm_bytes_per_launch"]
                    traffic_source = os.path.relpath(cand, ROOT) + " (PMC run of this build, lib_sha16 %s)" % lib_sha
                    break
        except Exception:
            traffic = None
        roofline = {"bound": "mfma", "achieved": achieved, "peak": MFMA_BF16_PEAK_TFLOPS, "unit": "TFLOP/s",
                    "frac": achieved / MFMA_BF16_PEAK_TFLOPS, "traffic": traffic, "traffic_source": traffic_source,
                    # the same algorithmic 3x3 FLOPs over the WHOLE timed step (everything else the step does included)
                    "whole_step_frac": conv3_fl * world / (dt / args.steps) / 1e12 / (MFMA_BF16_PEAK_TFLOPS * world),
                    "measured_in": ("the schedule `value` is timed on, instrumented: HIP events around every 3x3-conv launch on its own stream; "
                                    + ("forward launches alone on the chip, in the backward pass one backward-data launch (main stream) beside "
                                       "one weight-gradient launch per layer (side stream), each planned for its share of the CUs; "
                                       if two_streams else "one stream, every launch alone on the chip; ")
                                    + "achieved = algorithmic FLOPs / sum over launches of (duration x share of the 256 CUs the launch plans for)"),
                    "kernel": "3x3 conv MFMA kernels: igemm_pp / igemm_fwd2 (forward, backward-data) + igemm_wgpp / igemm_wgrad / igemm_wg_group (weight gradient)",
                    "timed_schedule_pass": {"attempts": attempts, "plausible": bool(plausible)},
                    "launches_per_step": n_launch // nprof,
                    "avg_launch_us": sum(v["wall_ms_per_step"] for v in prof_timed["by_kernel"].values()) / max(1, n_launch // nprof) * 1e3,
                    "conv_chip_ms_per_step": conv_t / nprof * 1e3,
                    # `frac` prices a launch by the CUs it PLANS for, so it can only overstate when the two backward streams do not overlap
                    # perfectly (a half-chip launch beside an idle queue, an unconfined split-K launch): it is an UPPER bound of the
                    # kernels' efficiency. The lower bound bills the whole chip whenever at least one 3x3-conv launch is running (union
                    # of the launches' busy intervals over both streams); `whole_step_frac` bills it for the whole step.
                    "frac_busy_union": conv_fl / prof_timed["busy_union_s"] / 1e12 / MFMA_BF16_PEAK_TFLOPS if prof_timed["busy_union_s"] > 0 else None,
                    "conv_busy_union_ms_per_step": prof_timed["busy_union_s"] / nprof * 1e3,
                    "algorithmic_gflop_per_step": conv_fl / nprof / 1e9,
                    "by_kernel": prof_timed["by_kernel"],
                    # every launch alone on the chip, one stream (no CU shares: chip time == wall time)
                    "frac_serial_per_layer": prof_serial["achieved"] / MFMA_BF16_PEAK_TFLOPS,
                    "by_kernel_serial_per_layer": prof_serial["by_kernel"],
                    "frac_single_stream_grouped": prof_grouped["achieved"] / MFMA_BF16_PEAK_TFLOPS,
                    "by_kernel_single_stream_grouped": prof_grouped["by_kernel"]}

    out = {
        "metric": "388x388 patches/sec fwd+bwd (1/2/4/8 GPU) + conv MFMA % of peak",
        "value": world * B * args.steps / dt,
        "unit": "patches/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": dt / args.steps * 1e3,
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "bf16",
        "data": "synthetic",
        "config": {"workload": "U-Net fwd+bwd+momentum step, num_layers=%d root_size=%d patch_size=%d input=%d%s" %
                               (L, root, P, S, " dilated" if args.dilated_layers else ""),
                   "batch_per_gpu": B, "global_batch": B * world, "parallelism": "dp%d" % world,
                   "step_tflops_algorithmic": tot_fl * world * args.steps / dt / 1e12, "loss": loss,
                   "dp_exchange": (None if bucketer is None else
                                   {"overlapped_buckets": bool(bucketer.overlap), "backward_cu_budget": m.backward_cu_budget or 256,
                                    "min_bucket_MB": bucketer.min_bucket * 4 >> 20,
                                    "schedule": ("tail-first buckets overlapped with backward" if bucketer.overlap else
                                                 "one all-reduce behind backward"),
                                    "exchange_proof": dp_proof,
                                    "tuned_ms_per_step": None if dp_tune is None else {
                                        "%s/%dcu/%dMB" % ("overlapped" if k[0] else "single", k[1], k[2] * 4 >> 20): v
                                        for k, v in dp_tune["ms"].items()}})},
        "roofline": roofline,
    }
    if sustained is not None:
        out["sustained"] = sustained
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        try:
            from oracle import torch_ref
            from oracle import unet_oracle as U
            tp = 132 if args.cpu_sample_patch > 132 else args.cpu_sample_patch   # bounded: ~10-20 s of oneDNN work on a big host
            tS = U.input_size_needed(tp, L)
            rng = np.random.RandomState(2017)
            Xs = rng.rand(1, tS, tS, 3).astype(np.float32)
            ls = (rng.rand(1, tp, tp) < 0.2).astype(np.int64)
            threads = physical_cores()
            tdt, _ = torch_ref.timed_train_step_fp32(U.init_params(L, root, False, seed=2018), Xs, ls, L, root, False, threads=threads, repeats=3)
            s_fl, _ = net_flops(L, root, False, tp, 1)
            f_fl, _ = net_flops(L, root, False, P, 1)
            model = ""
            try:
                model = [l.split(":", 1)[1].strip() for l in open("/proc/cpuinfo") if l.startswith("model name")][0]
            except Exception:
                pass
            out["cpu_baseline_torch"] = {"value": (s_fl / f_fl) / tdt, "unit": "patches/s", "cores": threads, "kind": "stand-in",
                                         "cpu_model": model, "gflops": s_fl / tdt / 1e9,
                                         "sample": "stock PyTorch-CPU float32 (oneDNN; oracle/torch_ref.py), fwd+bwd+momentum steps of "
                                                   "the same network on one %dx%d-output patch (input %d) = %.1f GFLOP: one warm-up step, then "
                                                   "the best of 3 = %.2f s, scaled by algorithmic FLOPs to 388-patch equivalents; "
                                                   "TensorFlow 1.4 cannot be installed" %
                                                   (tp, tp, tS, s_fl / 1e9, tdt)}
        except Exception as ex:
            out["cpu_baseline_torch"] = {"value": None, "unit": "patches/s", "kind": "stand-in", "sample": "failed: %r" % (ex,)}
        try:
            cdt, cS, cthreads = cpu_baseline(L, root, args.cpu_sample_patch, physical_cores())
            sample_fl, _ = net_flops(L, root, False, args.cpu_sample_patch, 1)
            full_fl, _ = net_flops(L, root, False, P, 1)
            out["cpu_baseline"] = {"value": (sample_fl / full_fl) / cdt, "unit": "patches/s", "cores": cthreads, "kind": "port",
                                   "sample": "oracle/unet_oracle.c (OpenMP on the physical cores, fp32 data / fp64 accumulate), fwd+bwd+momentum "
                                             "steps of the same L=%d root=%d network on one %dx%d-output patch (input %d) = %.1f GFLOP: one "
                                             "warm-up step on a small patch, then the best of 2 = %.1f s, scaled by algorithmic FLOPs to "
                                             "388-patch equivalents" %
                                             (L, root, args.cpu_sample_patch, args.cpu_sample_patch, cS, sample_fl / 1e9, cdt),
                                   "gflops": sample_fl / cdt / 1e9}
        except Exception as ex:  # the baseline is reported, never required for the GPU number
            out["cpu_baseline"] = {"value": None, "unit": "patches/s", "cores": os.cpu_count(), "kind": "port", "sample": "failed: %r" % (ex,)}
    if rank == 0:
        print(json.dumps(out))
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
