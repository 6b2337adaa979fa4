#!/usr/bin/env python3
"""Headline benchmark: points/sec, forward + backward, PointNet++ SemSeg, B=16 x 4096 x (3+6) per GPU.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--workload msg|ssg|sa] [--dump-outputs DIR] [--full [--no-cpu-baseline]]

One "step" = one pass of the hot path over one batch of synthetic KITTI-shaped clouds already resident in
HBM: forward (SA/FP stack + head), nll_loss over all B*N points (reference semseg.py:141-143), backward,
and -- for N > 1 -- the flat gradient all-reduce (RCCL).  Optimizer step excluded.
Train mode (BatchNorm batch statistics), fp32, dropout as in the reference (p = 0.5 in the head).

For N > 1 the driver launches one rank per GPU through torch.distributed.run; every rank owns its own 16
clouds (weak scaling, global batch 16*N) and the only collective is the gradient all-reduce.

Rank 0 prints ONE JSON line.  A plain run sets up, warms up, times exactly K steps and prints the headline
(``value``, ``ms_per_step``).  ``--dump-outputs DIR`` also writes what the last timed step returned (loss and log-probs,
or the SA module's outputs; bit-identical run to run) as DIR/<name>.npy.  ``--full`` adds everything that takes runs of
its own: ``roofline`` / ``kernels`` (the kernel family that takes the most device time, timed live with HIP events
around every C-ABI launch in an instrumented pass after the timed region), ``cpu_baseline`` (the oracle, a torch-CPU
port of the reference path in oracle/, timed on this host's cores on a bounded sample of the same workload) and, for
the default configuration, ``other_configs`` (the other BASELINE.json configurations, each a child run of this script).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
# RCCL between processes needs dmabuf IPC on this host driver (already exported on the GPU boxes; kept here so a bare
# `torch.distributed.run bench.py` works too).  Must be set before the HIP runtime loads.
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
# kernel arguments in device memory: the ROCm 7.2 default on gfx950; with 0 every launch of the replayed graph costs more
# (SSG step 2.96 -> 3.23 ms, MSG 7.34 -> 7.56 ms, measured) -- pinned so a differing site default cannot change the number
os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")

HBM_PEAK_GBS = 8000.0        # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
F32_MFMA_PEAK_TF = 157.3     # v_mfma_f32_32x32x2_f32 dense peak (= fp32 vector peak)
BF16_MFMA_PEAK_TF = 2500.0   # v_mfma_f32_32x32x16_bf16 dense peak (MI355X_MICROARCH.md)
SPLIT_PEAK_TF = BF16_MFMA_PEAK_TF / 6.0      # split kernels: six bf16 MFMAs per fp32 product block -> 416.7 TF of fp32 products
# C-ABI GEMM entry point -> kernel families of tools/pmc_traffic.py that serve it
GEMM_FAMILIES = {"pn2_conv1x1_bwd_pair": ["bwd_pair_kernel"],
                 "pn2_conv1x1_wgrad": ["gemm_tn_kernel", "wgrad_skinny_kernel", "wgrad_first_cf_kernel", "wgrad_full_kernel", "wgrad_reduce_kernel",
                                       "split_tn_kernel"],
                 "pn2_conv1x1_dgrad": ["gemm_nt_kernel<dgrad>", "regw_nt_kernel<dgrad>", "fewrow_nt_kernel<dgrad>", "split_nt_kernel<dgrad>"],
                 "pn2_conv1x1_bwd": ["gemm_bwd_fused_kernel"],     # (bwd_res_kernel + split_bwd_res_kernel: tools/pmc_traffic.py)
                 "pn2_conv1x1_fwd": ["gemm_nt_kernel<fwd>", "fwd_res_kernel", "regw_nt_kernel<fwd>", "fewrow_nt_kernel<fwd>", "split_nt_kernel<fwd>"]}

WORKLOADS = {
    "msg": "PointNet2 MSG SemSeg (SetAbstractionMsg 3 radii + FeaturePropagation), B=16x4096x(3+6), fwd+bwd",
    "ssg": "PointNet2SemSeg (reference SSG, model/pointnet2.py:141-176), B=16x4096x(3+6), fwd+bwd",
    "sa": "single PointNetSetAbstraction(1024,0.1,32,9,[32,32,64]), B=8x4096, fwd+bwd",
}


def algorithmic_work(name, a):
    """(flops, bytes) one C-ABI launch has to do at minimum, from its arguments (fp32 = 4 B, idx = 8 B)."""
    if name in ("pn2_conv1x1_fwd", "pn2_conv1x1_fwd_pool"):            # X ldx aff W ldw bias Y ldy P K N stats stream
        P, K, N = a[8], a[9], a[10]
        if a[6] is None:                     # (pooled last layer without an output: Y == NULL)
            return 2.0 * P * K * N, 4.0 * (P * K + N * K)
        return 2.0 * P * K * N, 4.0 * (P * K + P * N + N * K)
    if name == "pn2_conv1x1_dgrad":          # ... P K N stream   (reads dZ|pooled + Y [P,K], writes [P,N], reads prev_Y)
        P, K, N = a[17], a[18], a[19]
        dense = a[0] is not None
        masked = a[11] is not None
        return 2.0 * P * K * N, 4.0 * (P * K * (2 if dense else 1) + P * N * (2 if masked else 1) + N * K)
    if name == "pn2_conv1x1_wgrad":          # ... P M N stream
        P, M, N = a[15], a[16], a[17]
        dense = a[0] is not None
        return 2.0 * P * M * N, 4.0 * (P * M * (2 if dense else 1) + P * N + M * N)
    if name == "pn2_conv1x1_wgrad_cf":       # dZ ldz coef X ldx W ldw bias mom dW lddw P M N: closed-form BatchNorm terms, Y not read
        P, M, N = a[11], a[12], a[13]          # (booked with the bytes THIS formulation needs, not the general one's P*M more)
        if a[0] is None:                     # (dZ^T x came from the next layer's fused backward: this pass reads the input rows only)
            return 2.0 * P * N * N, 4.0 * (P * N + M * N)
        return 2.0 * P * M * N, 4.0 * (P * M + P * N + M * N)
    if name == "pn2_conv1x1_bwd_first":      # fused backward that also forms the first layer's dZ^T x: dZ, Y, prev_Y, X0 read; NO dX written
        P, Co, Ci, N0 = a[17], a[18], a[19], a[15]
        return 4.0 * P * Co * Ci + 2.0 * P * Ci * N0, 4.0 * (2 * P * Co + P * Ci + P * a[14] + 2 * Co * Ci)
    if name == "pn2_conv1x1_bwd_pair":       # dgrad + wgrad of one layer behind ONE grid: each body reads its own operands
        P, Co, Ci = a[22], a[23], a[24]
        dense, masked = a[0] is not None, a[11] is not None
        dy = P * Co * (2 if dense else 1)
        return 4.0 * P * Co * Ci, 4.0 * (dy + P * Ci * (2 if masked else 1) + Ci * Co) + 4.0 * (dy + P * Ci + Co * Ci)
    if name == "pn2_conv1x1_bwd":            # fused dgrad + wgrad: dZ|pooled, Y [P,Co], prev_Y [P,Ci] read once, dX [P,Ci] written
        P, Co, Ci = a[19], a[20], a[21]
        dense = a[0] is not None
        return 4.0 * P * Co * Ci, 4.0 * (P * Co * (2 if dense else 1) + 2 * P * Ci + 2 * Co * Ci)
    if name == "pn2_conv1x1_bwd_cf":         # pooled last layer from its input: prev_Y read, dX written (no Y stream); flops as the layer's
        P, Co, Ci = a[16], a[17], a[18]
        return 4.0 * P * Co * Ci, 4.0 * (2 * P * Ci + 2 * Co * Ci)
    if name == "pn2_bn_relu_max":            # Y ldy aff G K C out ldo arg
        G, K, C = a[3], a[4], a[5]
        return 3.0 * G * K * C, 4.0 * (G * K * C + 2 * G * C)
    if name == "pn2_group":                  # xyz points new_xyz idx B N S K D xyz_first ld out
        B, N, S, K, D, ld = a[4], a[5], a[6], a[7], a[8], a[10]
        return 0.0, 4.0 * B * S * K * (ld + 3 + D) + 8.0 * B * S * K
    if name == "pn2_group_bwd":
        B, N, S, K, D = a[2], a[3], a[4], a[5], a[6]
        return 0.0, 4.0 * B * S * K * D * 2 + 8.0 * B * S * K
    if name == "pn2_fps":                    # latency chain: bytes touched once if register resident
        B, N = a[1], a[2]
        return 10.0 * B * N * a[4], 12.0 * B * N
    if name == "pn2_ball_query":
        B, N, S, ns = a[2], a[3], a[4], a[6]
        return 11.0 * B * S * N, 12.0 * B * (N + S) + 8.0 * B * S * ns
    if name == "pn2_three_nn":
        B, N, S = a[2], a[3], a[4]
        return 14.0 * B * N * S, 12.0 * B * (N + S) + 48.0 * B * N
    return 0.0, 0.0


def kernel_key(name):
    """A kernel's name as both rocprofv3 (Kernel_Name / stats CSV) and pn2_last_kernel() spell it, minus what differs between
    the two: the return type, the anonymous-namespace qualifiers and the parameter list."""
    name = name.strip().replace("(anonymous namespace)::", "")
    if name.startswith("void "):
        name = name[5:]
    if name.endswith(")"):                        # parameter list: the parenthesis that closes last opens it
        depth = 0
        for i in range(len(name) - 1, -1, -1):
            depth += name[i] == ")"
            depth -= name[i] == "("
            if depth == 0:
                name = name[:i]
                break
    return name.strip()


def kernel_pipe(key):
    """Which matrix pipe a GEMM kernel of the library runs its products on: the bf16 pipe with exact three-way operand splits
    (six MFMAs per fp32 product block) or the fp32 MFMA."""
    return "bf16x3" if key.startswith("split_") else "f32"


def price(flops, nbytes, secs, pipe):
    """(bound, achieved, peak, unit, frac, hbm_frac, mfma_frac) of a kernel on the roofline that applies to it: HBM 8 TB/s on its
    ALGORITHMIC bytes against the matrix peak of ITS pipe on its algorithmic fp32 flops; the larger fraction names the bound."""
    gbs, tf = nbytes / secs / 1e9, flops / secs / 1e12
    peak_tf = SPLIT_PEAK_TF if pipe == "bf16x3" else F32_MFMA_PEAK_TF
    hf, mf = gbs / HBM_PEAK_GBS, (tf / peak_tf if pipe else 0.0)
    if mf > hf:
        return "mfma", round(tf, 3), round(peak_tf, 1), "TFLOP/s", round(mf, 4), round(hf, 4), round(mf, 4)
    return "hbm", round(gbs, 1), HBM_PEAK_GBS, "GB/s", round(hf, 4), round(hf, 4), round(mf, 4)


def csrc_digest():
    """sha256 over the kernel sources: stamps profiles/*_pmc_traffic_*.json so a stale file is never quoted."""
    import glob
    import hashlib
    h = hashlib.sha256()
    for f in sorted(glob.glob(os.path.join(ROOT, "pointnet12_amd", "csrc", "*.hip")) +
                    glob.glob(os.path.join(ROOT, "pointnet12_amd", "csrc", "*.h"))):
        h.update(os.path.basename(f).encode())
        h.update(open(f, "rb").read())
    return h.hexdigest()


def build_net(workload, dev, npoint_scale=1):
    import torch
    from pointnet12_amd import pointnet2 as M
    from pointnet12_amd import pointnet_util as U
    torch.manual_seed(0)
    if workload == "msg":
        net = M.PointNet2SemSegMsg(13, 6, npoint_scale=npoint_scale)
    elif workload == "ssg":
        net = M.PointNet2SemSeg(13, 6)
    else:
        net = U.PointNetSetAbstraction(1024, 0.1, 32, 9, [32, 32, 64], False)
    return net.to(dev).train()


# SURVEY.md section 8(d), per input point: (ALG_BYTES, FLOP) of one forward + backward step at N = 4096 points per cloud
STEP_MODEL = {"msg": (225604, 464.5e9 / 65536), "ssg": (55689, 92.8e9 / 65536), "sa": (20720, 5.28e9 / 32768)}
# cfg5 of BASELINE.json (dense scan, B=8 x 65 536): MSG with npoint x16 (ALG_BYTES 118.13 GB, 3 716 GFLOP per step) and the
# reference's SSG net with its fixed npoints (8.108 GB, 244.6 GFLOP), per input point
STEP_MODEL_CFG5 = {("msg", 16): (118.13e9 / 524288, 3716e9 / 524288), ("ssg", 1): (8.108e9 / 524288, 244.6e9 / 524288)}


def make_step(workload, net, pts, labels, bucket, prefetch=True):
    from pointnet12_amd.loss import nll_loss      # F.nll_loss (semseg.py:143) on the HIP library
    from pointnet12_amd import graph as _graph
    # Where the next batch's geometry branch (FPS / ball query / 3-NN of the NEXT batch, 0.55 ms of small grids at 4096 points)
    # starts inside the captured step.  Same-box A/B, ms per step (gpurun_out r5z, two repetitions each):
    #     fork at      top          behind sa1    behind sa2    behind the loss   at sa2's backward   at sa1's backward
    #     MSG          5.24 - 5.29  5.28 - 5.33   5.28 - 5.29   5.33 - 5.34       5.48 - 5.53         5.41 - 5.43
    #     SSG          2.49 - 2.50  2.49          2.47          2.53              2.95                3.17 - 3.19
    # (round 4 forked behind the loss: 5.84 -> 5.76 ms then.  The bf16-split GEMMs of this round are persistent workgroups that
    # fill a CU's register file -- nothing co-runs with them -- and under the backward chain's small kernels the branch's FPS
    # stretched the chain: rocprofv3 trace, tools/step_timeline.py.)  cfg2 / cfg5: the FPS chain is the step, top.
    # Round 6 (output-free pooled layers, two workgroups per CU): MSG forked behind sa2 4.964 - 5.005 against 5.010 - 5.049 at the top
    # (five alternating runs each, one box, gpurun_out r6u); SSG top / sa2 / loss equal within the run-to-run spread (2.46 - 2.50).
    default_fork = {"msg": "sa2", "ssg": "sa2"}.get(workload, "top") if pts.shape[-1] <= 8192 else "top"
    fork_at = os.environ.get("PN2_BENCH_FORK", default_fork)       # top | sa1 | sa2 | loss | sa2_bwd | sa1_bwd
    # (no geometry branch -- eager launches or --no-prefetch -- means nothing to fork: the step is the plain sequence)
    late_fork = prefetch and fork_at != "top" and workload in ("msg", "ssg")
    if not late_fork:
        fork_at = "top"
    if fork_at in ("sa1", "sa2"):                 # behind that module's forward
        getattr(net, fork_at).register_forward_hook(lambda m, i, o: _graph.fork_point())
    if fork_at in ("sa1_bwd", "sa2_bwd"):         # where the backward pass reaches that module (the gradient of its output features)
        def _hook_out(m, i, o):
            if o[1].requires_grad:
                o[1].register_hook(lambda g: (_graph.fork_point(), None)[1])
        getattr(net, fork_at[:3]).register_forward_hook(_hook_out)

    def step():
        """-> {name: tensor} of what a caller of the step receives besides the gradients (static tensors when captured)."""
        bucket.wait_reduced()                     # comm stream: the previous step's all-reduce (an event-wait node when captured)
        bucket.zero()
        if workload == "sa":
            new_xyz, feat = net(pts[:, :3, :], pts[:, 3:, :])
            loss = feat.sum()
            out = {"new_xyz": new_xyz, "features": feat}
        else:
            lp = net(pts)
            loss = nll_loss(lp.reshape(-1, lp.shape[-1]), labels.reshape(-1))
            out = {"log_probs": lp}
        if late_fork and fork_at == "loss":
            _graph.fork_point()                   # a captured step starts the next batch's geometry branch here
        loss.backward()
        out["loss"] = loss
        return out
    step.fork_in_step = late_fork                 # (GraphedStep: this step function calls graph.fork_point() itself)
    return step


def _cpu_info():
    """(model string, physical cores, logical cpus) of this host."""
    model, phys, cores_by_pkg = "unknown", set(), {}
    try:
        pkg = core = None
        for ln in open("/proc/cpuinfo"):
            k, _, v = ln.partition(":")
            k, v = k.strip(), v.strip()
            if k == "model name":
                model = v
            elif k == "physical id":
                pkg = v
            elif k == "core id":
                core = v
            elif not k and pkg is not None:
                phys.add((pkg, core))
                pkg = core = None
    except OSError:
        pass
    logical = os.cpu_count() or 1
    try:
        logical = len(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        pass
    n_phys = len(phys) if phys else logical
    return model, max(1, min(n_phys, logical)), logical


def cpu_baseline_slice(workload, batch, n_points, npoint_scale):
    """cfg5 (dense scans): the reference algorithm needs > 100 GB for the [8, 8192, 65536] int64 sort of a whole batch, so the
    CPU side runs ONE cloud (B = 1) with the reference's own ATen operator sequence and the result is extrapolated to the
    batch ("cfg5 on CPU runs cloud-by-cloud"; BatchNorm statistics are then per cloud, which changes
    no operator's cost).  One step, timed as it is (a second one would double a leg that already takes minutes)."""
    import torch
    from oracle import torch_ref as T
    from pointnet12_amd import synthetic as syn
    pts_np, lab_np = syn.kitti_batch(0, 1, n_points)
    pts, lab = torch.from_numpy(pts_np), torch.from_numpy(lab_np)
    T.set_geometry("aten")
    torch.manual_seed(0)
    net = T.RefMSGSemSeg(13, 6, npoint_scale=npoint_scale) if workload == "msg" else T.RefSSGSemSeg(13, 6)
    net.train()
    model, n_phys, logical = _cpu_info()
    # SSG: 8 threads as everywhere else (30 GFLOP per cloud: seconds).  MSG with npoint x16 is 464 GFLOP of conv / BatchNorm
    # per cloud -- a quarter of an hour at 8 threads -- so that leg uses every physical core of the host (stated in `cores`)
    threads = min(8, logical) if workload == "ssg" else n_phys
    saved = torch.get_num_threads()
    try:
        torch.set_num_threads(threads)
        torch.manual_seed(1234)
        t0 = time.perf_counter()
        net.zero_grad()
        T.seg_loss(net(pts), lab).backward()
        secs = time.perf_counter() - t0
    finally:
        torch.set_num_threads(saved)
        T.set_geometry("c")
    return {"value": round(n_points / secs, 1), "unit": "points/s", "cores": threads, "kind": "port", "physical_cores": n_phys,
            "logical_cpus": logical, "cpu_model": model, "s_per_cloud": round(secs, 2), "s_per_step_extrapolated": round(secs * batch, 1),
            "sample": "ONE cloud of the batch (B=1 x %d pts; the reference's dense [B,S,N] matrices do not fit a whole batch), oracle "
                      "net of oracle/torch_ref.py with the reference's ATen operator sequence for FPS / ball query / 3-NN, train mode, "
                      "one cold step at %d threads; the batch of %d clouds costs %d x this" % (n_points, threads, batch, batch)}


def cpu_baseline(workload, batch, budget_s=150.0):
    """The reference's CPU path, as restated by the oracle with the reference's own operator sequence for the
    geometry (oracle/aten_geometry.py), on the FULL benchmark batch, timed twice: with 8
    threads (comparable with the survey container's reference timings) and with all physical cores of this host.
    1 warm-up + median of 3 steps each (fewer when a step is so slow that the leg would pass `budget_s`)."""
    import numpy as np
    import torch
    from oracle import torch_ref as T
    from pointnet12_amd import synthetic as syn
    pts_np, lab_np = syn.kitti_batch(0, batch, 4096)
    pts, lab = torch.from_numpy(pts_np), torch.from_numpy(lab_np)
    T.set_geometry("aten")
    torch.manual_seed(0)
    if workload == "msg":
        net = T.RefMSGSemSeg(13, 6)
    elif workload == "ssg":
        net = T.RefSSGSemSeg(13, 6)
    else:
        net = T.RefSetAbstraction(1024, 0.1, 32, 9, [32, 32, 64], False)
    net.train()

    def step():
        net.zero_grad()
        if workload == "sa":
            _, f = net(pts[:, :3, :], pts[:, 3:, :])
            f.sum().backward()
        else:
            T.seg_loss(net(pts), lab).backward()

    model, n_phys, logical = _cpu_info()
    saved = torch.get_num_threads()
    legs = {}
    try:
        for threads in sorted({min(8, logical), n_phys}):
            torch.set_num_threads(threads)
            torch.manual_seed(1234)
            t0 = time.perf_counter()
            step()                                   # warm-up
            warm = time.perf_counter() - t0
            left = budget_s / 2 - warm               # each of the two legs gets half of the budget
            n_timed = int(max(1, min(3, left // max(warm, 1e-3))))
            times = []
            for _ in range(n_timed):
                t0 = time.perf_counter()
                step()
                times.append(time.perf_counter() - t0)
            legs[threads] = (float(np.median(times)), n_timed)
    finally:
        torch.set_num_threads(saved)
        T.set_geometry("c")
    best = min(legs, key=lambda k: legs[k][0])
    rate = lambda th: round(batch * 4096 / legs[th][0], 1)
    t8 = min(8, logical)
    return {"value": rate(best), "unit": "points/s", "cores": best, "kind": "port",
            "value_8t": rate(t8), "value_all_cores": rate(n_phys), "physical_cores": n_phys, "logical_cpus": logical,
            "cpu_model": model, "s_per_step": {str(k): round(v[0], 3) for k, v in legs.items()},
            "timed_steps": {str(k): v[1] for k, v in legs.items()},
            "sample": "the whole benchmark batch (B=%d x 4096 pts), oracle net of oracle/torch_ref.py with the reference's "
                      "ATen operator sequence for FPS / ball query / 3-NN (oracle/aten_geometry.py) and torch-CPU "
                      "conv/BatchNorm, train mode; 1 warm-up + median of the timed steps, at %s threads" % (
                          batch, " and ".join(str(k) for k in sorted(legs)))}


def rccl_env(rank):
    """Pin the collective's transport to the node and make RCCL say what it picked (VERDICT r3 #7a).  Set BEFORE the process
    group comes up: InfiniBand / RoCE off and the bootstrap socket on loopback (one node: the data path can then only be
    xGMI / PCIe peer-to-peer or host shared memory -- which of them is read back from RCCL's own log), NCCL_DEBUG=INFO into one
    file per rank (a file, not stdout: stdout carries the ONE JSON line)."""
    import tempfile
    os.environ["NCCL_IB_DISABLE"] = "1"
    os.environ.setdefault("NCCL_SOCKET_IFNAME", "lo")
    os.environ.setdefault("NCCL_DEBUG", "INFO")
    log = os.environ.get("NCCL_DEBUG_FILE")
    if not log:
        d = os.environ.get("PN2_RCCL_LOG_DIR") or tempfile.mkdtemp(prefix="pn2_rccl_")
        os.makedirs(d, exist_ok=True)
        log = os.path.join(d, "rccl_rank%d.log" % rank)
        os.environ["NCCL_DEBUG_FILE"] = log
    return log


def parse_rccl_log(path):
    """{"version", "channels": {transport: count}, "net_plugin", "rings"} from one rank's NCCL_DEBUG=INFO file; never raises."""
    import re
    out = {"log": path, "version": None, "channels": {}, "net": None, "rings": 0, "trees": 0}
    try:
        text = open(path, errors="replace").read()
    except OSError as e:
        out["error"] = str(e)
        return out
    m = re.search(r"(RCCL version[^\n]*|NCCL version[^\n]*)", text)
    if m:
        out["version"] = m.group(1).strip()[:120]
    for m in re.finditer(r"Channel \d+/\d+ *: *\d+\[[^\]]*\] *-> *\d+\[[^\]]*\].* via (\S+)", text):
        t = m.group(1)
        out["channels"][t] = out["channels"].get(t, 0) + 1
    m = re.search(r"Using network (\S+)", text)
    if m:
        out["net"] = m.group(1)
    out["rings"] = len(re.findall(r"\bRing \d+ *:", text))
    out["trees"] = len(re.findall(r"\bTrees? \[", text))
    return out


def self_launch(n):
    """`python bench.py --gpus N` without a launcher: start the N ranks through torch.distributed.run as a CHILD process
    (this parent never touches the GPU: no re-exec of a process that has initialised HIP), relay rank 0's JSON line
    and the return code."""
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    proc = subprocess.Popen(cmd, stdout=subprocess.PIPE, text=True)
    lines = []
    for ln in proc.stdout:
        if ln.startswith("{") and '"metric"' in ln:
            lines.append(ln.strip())
        else:
            sys.stderr.write(ln)
    rc = proc.wait()
    if lines:
        print(lines[-1])
    sys.exit(rc if rc else (0 if lines else 1))


def timed_protocol(step, all_reduce, fence, steps, warmup, world, dist, torch, dev=None):
    """The rank protocol of the benchmark, shared by the real run and --dry-run: W untimed steps, fence (barrier + device
    synchronise), exactly K timed steps, fence; every step = ``step()`` followed by the gradient ``all_reduce()``.  Returns
    (elapsed of the SLOWEST rank, {"allreduce_ms", "rank_ms_per_step_min", "rank_ms_per_step_max"}): the collective is
    timed on its own (HIP events on the stream it is issued from; wall clock on CPU) so that a scaling loss at N GPUs
    can be attributed to it, and the per-rank spread shows a straggler."""
    use_events = dev is not None
    for _ in range(warmup):
        step()
        all_reduce()
    fence()
    marks = []
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
        if use_events:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            own = all_reduce()                   # a collective on a comm stream brings its own pair of events
            e1.record()
            marks.append(own if isinstance(own, tuple) else (e0, e1))
        else:
            a = time.perf_counter()
            all_reduce()
            marks.append(time.perf_counter() - a)
    fence()
    elapsed = time.perf_counter() - t0
    ar_ms = sum(e0.elapsed_time(e1) for e0, e1 in marks) if use_events else sum(marks) * 1e3
    info = {"allreduce_ms": round(ar_ms / max(steps, 1), 4)}
    mine = elapsed / max(steps, 1) * 1e3
    if world > 1:
        t = torch.tensor([elapsed, -elapsed, ar_ms / max(steps, 1)], dtype=torch.float64, device=dev if use_events else None)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t[0].item())
        info["rank_ms_per_step_min"] = round(-float(t[1].item()) / max(steps, 1) * 1e3, 3)
        info["rank_ms_per_step_max"] = round(elapsed / max(steps, 1) * 1e3, 3)
        info["allreduce_ms"] = round(float(t[2].item()), 4)                # the slowest rank's
    else:
        info["rank_ms_per_step_min"] = info["rank_ms_per_step_max"] = round(mine, 3)
    return elapsed, info


DUMP_LIMIT_BYTES = 60 << 20      # --dump-outputs: array data in all (the .npy headers stay well inside 64 MB)


def dump_outputs(out_dir, arrays):
    """{name: tensor} -> out_dir/<name>.npy in float32 (float64 stays float64).  When the whole would pass DUMP_LIMIT_BYTES, an
    array larger than its even share of what is left is written as a fixed, seeded sample of its flattened elements (sorted
    positions, the same on every run of the same arguments); stderr says which."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    host = {}
    for name, t in arrays.items():
        a = t.detach().cpu().numpy()
        host[name] = a if a.dtype == np.float64 else a.astype(np.float32)
    left = DUMP_LIMIT_BYTES
    order = sorted(host, key=lambda n: (host[n].nbytes, n))
    for i, name in enumerate(order):
        a = host[name]
        share = left // (len(order) - i)
        if a.nbytes > share:
            k = share // a.itemsize
            a = a.reshape(-1)[np.sort(np.random.default_rng(0).choice(a.size, k, replace=False))]
            print("bench: %s.npy holds a seeded sample of %d of its %d elements" % (name, k, host[name].size), file=sys.stderr)
        np.save(os.path.join(out_dir, name + ".npy"), a)
        left -= a.nbytes


def dry_run(args, dist, torch):
    """The benchmark's rank protocol on CPU with gloo ranks and no GPU: the same ``timed_protocol`` as the real run around a toy
    conv + BatchNorm network (plain torch; nothing of oracle/ -- that is for the cpu_baseline legs only) accumulating into the
    real ``parallel.FlatGradBucket`` (autograd mode) and its all-reduce -- rendezvous on 127.0.0.1, barrier, K timed steps, MAX
    over ranks, one JSON line from rank 0 relayed by the parent (tests/test_bench_launch_cpu.py)."""
    from pointnet12_amd import parallel
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d" % (args.gpus, world))
    if world > 1:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(1)
    per_rank = 2
    lo, _ = parallel.shard_range(per_rank * world, rank, world)
    gen = torch.Generator().manual_seed(20260101 + lo)           # every rank its own clouds (the shard's first cloud index seeds them)
    pts = torch.randn(per_rank, 9, 256, generator=gen)
    lab = torch.randint(0, 13, (per_rank, 256), generator=gen)
    torch.manual_seed(rank)                          # different initial parameters per rank: the broadcast must fix that
    nn = torch.nn
    net = nn.Sequential(nn.Conv1d(9, 32, 1), nn.BatchNorm1d(32), nn.ReLU(), nn.Conv1d(32, 64, 1), nn.BatchNorm1d(64), nn.ReLU(),
                        nn.Conv1d(64, 13, 1)).train()
    parallel.broadcast_module(net)
    bucket = parallel.FlatGradBucket(net, direct=False)

    def step():
        bucket.zero()
        torch.nn.functional.cross_entropy(net(pts), lab).backward()
        time.sleep(0.002 * rank)                     # uneven ranks: the reported time must be the slowest one's

    def fence():
        if world > 1:
            dist.barrier()

    elapsed, info = timed_protocol(step, bucket.all_reduce, fence, args.steps, args.warmup, world, dist, torch)
    # every rank now holds the same averaged bucket and the same parameters
    digest = torch.tensor([float(bucket.flat.double().abs().sum()), float(sum(p.double().abs().sum() for p in net.parameters()))],
                          dtype=torch.float64)
    same = True
    if world > 1:
        hi, lo_ = digest.clone(), digest.clone()
        dist.all_reduce(hi, op=dist.ReduceOp.MAX)
        dist.all_reduce(lo_, op=dist.ReduceOp.MIN)
        same = bool(((hi - lo_).abs() <= 1e-9 * hi.abs()).all())
        dist.destroy_process_group()
    if rank == 0:
        line = {"metric": "points/sec fwd+bwd, PointNet2 SemSeg B=16x4096 pts", "value": 0.0, "unit": "points/s",
                "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
                "ms_per_step": round(elapsed / max(args.steps, 1) * 1e3, 3), "dry_run": True,
                "ranks_agree": same, "grad_bucket_bytes": bucket.nbytes}
        line.update(info)
        print(json.dumps(line))


OTHER_CONFIGS = [   # name, extra arguments (the headline, cfg3 MSG, is the run that prints them)
    ("cfg3_ssg_B16x4096", ["--workload", "ssg"]),
    ("cfg2_sa_B8x4096", ["--workload", "sa"]),
    ("cfg5_ssg_B8x65536", ["--workload", "ssg", "--points", "65536", "--batch", "8", "--steps", "10", "--warmup", "3"]),
    ("cfg5_msg_B8x65536_npoint_x16", ["--workload", "msg", "--points", "65536", "--batch", "8", "--npoint-scale", "16", "--steps", "5",
                                      "--warmup", "2"]),
]


def other_configs():
    """{name: {ms_per_step, points_per_s, step_hbm_frac, step_mfma_frac, ...}} of the configurations the headline line does not
    time: each one is this script again as a CHILD process (its own allocator pool; the parent never execs), with the same
    timed protocol (barrier + synchronize around exactly --steps replays), without the CPU baseline."""
    import subprocess
    out = {}
    for name, extra in OTHER_CONFIGS:
        cmd = [sys.executable, os.path.abspath(__file__)] + extra + ["--full", "--no-cpu-baseline", "--no-other-configs"]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
            doc = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
            sr = doc.get("step_roofline") or {}
            out[name] = {"ms_per_step": doc["ms_per_step"], "points_per_s": doc["value"], "steps": doc["steps"], "warmup": doc["warmup"],
                         "step_hbm_frac": sr.get("hbm_frac"), "step_mfma_frac": sr.get("mfma_frac"),
                         "step_mfma_frac_reference_formulation": sr.get("mfma_frac_reference_formulation"),
                         "workload": doc["config"]["workload"], "clouds": doc["config"]["clouds_per_gpu"],
                         "points_per_cloud": doc["config"]["points_per_cloud"]}
        except Exception as e:                         # a failed side run must not take the headline line down with it
            out[name] = {"error": repr(e)[:200]}
    # the reference viewer's single-cloud forward (pcdvis.py:118-136, model/utils.py:15-34) -- PointNet2SemSeg(19, 1) in
    # eval mode on ONE 25 000-point cloud, the fused eval path (pn2_fused_eval); latency of one frame as a hipGraph replay, and the
    # time per frame of a frame stream with the next frame's geometry prefetched (tools/bench_infer.py, a child process as above)
    try:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bench_infer.py"), "--points", "25000", "--reps", "50"],
                           capture_output=True, text=True, timeout=300)
        doc = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
        out["infer_single_cloud_25000_eval"] = {"latency_ms_graph": doc["graph_ms"], "latency_ms_eager": doc["eager_ms"],
                                                "stream_ms_per_frame": doc["stream_ms_per_frame"], "points_per_s": doc["points_per_s"],
                                                "workload": "PointNet2SemSeg(19, 1) eval forward, 1 x 25000 x 4 (pcdvis.py:118-136)",
                                                "fps_ms": doc["kernels_ms"].get("pn2_fps")}
    except Exception as e:
        out["infer_single_cloud_25000_eval"] = {"error": repr(e)[:200]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--workload", choices=sorted(WORKLOADS), default="msg")
    ap.add_argument("--batch", type=int, default=0, help="clouds per GPU (default 16; 8 for --workload sa)")
    ap.add_argument("--points", type=int, default=4096, help="points per cloud (cfg5 of BASELINE.json: 65536)")
    ap.add_argument("--npoint-scale", type=int, default=1, help="MSG only: multiply sa1/sa2 npoint (cfg5: 16)")
    ap.add_argument("--full", action="store_true",
                    help="after the headline, also the instrumented roofline pass, the CPU baseline and (default configuration) the "
                         "other BASELINE.json configurations; a plain run does none of them")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="write what the last timed step returned (loss and log-probs, or the SA module's outputs) as DIR/<name>.npy")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-roofline", action="store_true", help="with --full: skip the instrumented roofline pass")
    ap.add_argument("--detail", action="store_true", help="with --full: per-launch table of the instrumented pass on stderr")
    ap.add_argument("--no-comm-stream", action="store_true", help="issue the gradient all-reduce on the step's own stream")
    ap.add_argument("--no-two-bucket", action="store_true",
                    help="one all-reduce of the whole bucket behind the step instead of early (under sa1's backward) + late")
    ap.add_argument("--no-graph", action="store_true", help="launch every kernel eagerly instead of replaying a hipGraph")
    ap.add_argument("--no-prefetch", action="store_true",
                    help="compute each batch's FPS/ball-query/3-NN inside its own step instead of one step ahead")
    ap.add_argument("--no-other-configs", action="store_true",
                    help="with --full: skip the short runs of the other BASELINE.json configurations (other_configs)")
    ap.add_argument("--same-device", action="store_true",
                    help="testing only: every rank uses GPU 0 (a one-GPU box exercising the N > 1 RCCL path, if RCCL accepts two ranks "
                         "on one device)")
    ap.add_argument("--dry-run", action="store_true",
                    help="CPU only: exercise the launch / rendezvous / max-over-ranks timing / JSON relay with gloo ranks "
                         "and no GPU work (tests/test_bench_launch_cpu.py)")
    args = ap.parse_args()

    if args.gpus > 1 and "RANK" not in os.environ:
        self_launch(args.gpus)                       # never returns

    import numpy as np
    import torch
    import torch.distributed as dist
    if args.dry_run:
        return dry_run(args, dist, torch)
    from pointnet12_amd import _lib, parallel
    from pointnet12_amd import synthetic as syn

    rank = int(os.environ.get("RANK", "0"))
    local = 0 if args.same_device else int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d: launch with torch.distributed.run --nproc-per-node %d"
                         % (args.gpus, world, args.gpus))
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    use_dist = world > 1 or "RANK" in os.environ          # launched by torch.distributed.run (also with one rank)
    if use_dist:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29511")
        # RCCL prints its version banner on stdout when NCCL_DEBUG=VERSION is set in the environment: keep stdout
        # for the ONE JSON line by pointing fd 1 at stderr while the communicator comes up.
        rccl_log = rccl_env(rank)
        sys.stdout.flush()
        saved_stdout = os.dup(1)
        os.dup2(2, 1)
        try:
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
            warm = torch.zeros(1 << 20, device=dev)          # 4 MB: the size class of the gradient bucket (same channels / protocol)
            dist.all_reduce(warm)
            torch.cuda.synchronize()
        finally:
            os.dup2(saved_stdout, 1)
            os.close(saved_stdout)
    _lib.load()                              # no HIP library -> raise, never fall back
    split_on = bool(_lib.options().get("PN2_SPLIT", 0))      # wide-layer products on the bf16 pipe (see the JSON line's config)

    batch = args.batch or (8 if args.workload == "sa" else 16)
    n_points = args.points
    lo, _ = parallel.shard_range(batch * world, rank, world)
    pts_np, lab_np = syn.kitti_batch(lo, batch, n_points)
    pts = torch.from_numpy(pts_np).to(dev)
    labels = torch.from_numpy(lab_np).to(dev)

    rccl = None
    if use_dist:
        # every rank must own DIFFERENT clouds (weak scaling): the first cloud index of every rank, gathered and checked
        mine = torch.tensor([lo], dtype=torch.int64, device=dev)
        every = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(every, mine)
        los = [int(t.item()) for t in every]
        if len(set(los)) != world or sorted(los) != [batch * r for r in range(world)]:
            raise SystemExit("ranks do not own disjoint cloud shards: first cloud index per rank = %s" % los)
        rccl = {"ranks": world, "ib_disabled": os.environ.get("NCCL_IB_DISABLE") == "1",
                "socket_ifname": os.environ.get("NCCL_SOCKET_IFNAME"), "first_cloud_per_rank": los}
        rccl.update(parse_rccl_log(rccl_log))
        ch = rccl.get("channels") or {}
        rccl["transport"] = ("none (one rank: no peer)" if world == 1 else
                             (" + ".join("%s x%d" % kv for kv in sorted(ch.items())) or None))
        # "xGMI only" = every channel is GPU peer-to-peer (P2P/IPC, P2P/direct ...): no NET/*, no SHM hop through host memory
        rccl["peer_to_peer_only"] = bool(ch) and all(k.upper().startswith("P2P") for k in ch) if world > 1 else None

    net = build_net(args.workload, dev, args.npoint_scale)
    parallel.broadcast_module(net)
    bucket = parallel.FlatGradBucket(net, direct=True)
    comm_ok = None
    if use_dist and not args.no_comm_stream:
        # the comm-stream path has to EARN its place on this very process group before it is used for the timed steps
        # (ADVICE r3): one bucket of rank-dependent values through both paths, results compared bit for bit on every rank
        comm_ok = parallel.verify_comm_stream(bucket)
        if comm_ok:
            bucket.use_comm_stream()         # the all-reduce on its own stream, under the next replay's geometry branch
    two_bucket, two_detail = False, None
    if bucket.comm is not None and not args.no_two_bucket and args.workload in ("msg", "ssg") and not args.no_graph:
        # early bucket (everything but sa1) all-reduced UNDER sa1's backward, behind an event recorded inside the graph; the
        # mechanism is checked on this device first (a wait that binds to an older record would reduce unfinished gradients)
        two_bucket, two_detail = parallel.verify_in_graph_record(dev)
        if two_bucket:
            bucket.use_two_buckets(list(net.sa1.parameters()))
            bucket.arm(net.sa1)
    compute = make_step(args.workload, net, pts, labels, bucket,     # zero grads + forward + loss + backward
                        prefetch=not (args.no_graph or args.no_prefetch))
    if not args.no_graph:
        from pointnet12_amd.graph import GraphedStep
        torch.manual_seed(4321)
        geometry = None
        if not args.no_prefetch:                    # geometry-only pass (recording tape) over the next batch
            geometry = (lambda: net(pts[:, :3, :], pts[:, 3:, :])) if args.workload == "sa" else (lambda: net.features(pts))
        # (fork_in_step: the geometry branch starts at make_step's fork_point() where that pays -- see make_step)
        graphed = GraphedStep(compute, dev, geometry_fn=geometry,     # one hipGraph launch per step (failures raise)
                              fork_in_step=getattr(compute, "fork_in_step", False) and geometry is not None)
    else:
        graphed = compute

    def fence():
        if use_dist:
            dist.barrier()
        torch.cuda.synchronize()

    last = {}

    def timed_step():
        last["out"] = graphed()              # (the two alternating graphs own different output tensors: keep this replay's)

    torch.manual_seed(1234)                  # FPS start draws
    # one step = the graph replay, then the only collective of the path (no-op on one GPU), issued right behind it
    elapsed, rank_info = timed_protocol(timed_step, bucket.all_reduce_timed, fence, args.steps, args.warmup, world if use_dist else 1,
                                        dist, torch, dev)
    ms_per_step = elapsed / args.steps * 1e3
    value = batch * world * n_points * args.steps / elapsed

    if rank == 0 and args.dump_outputs:
        # the last timed step as its caller receives it: what the step returns (loss, log-probs / SA outputs), bit-identical run to
        # run.  The parameter gradients are not written: the backward's fp32 atomics ("What is reproducible run to
        # run") make them differ between runs of the same build, and those whose exact value is zero (a bias in front of a
        # training-mode BatchNorm) hold rounding residue only -- no two runs could be compared on them.
        dump_outputs(args.dump_outputs, last["out"])

    roofline = None
    kernels = None
    if rank == 0 and args.full and not args.no_roofline:
        # instrumented pass: HIP events around every C-ABI launch, on the stream the kernel runs on.  The launches
        # are issued one after the other here (no parallel MSG scale streams), so a launch's duration
        # is its own and not that of whatever shared the chip with it in the timed, overlapped step above.
        from pointnet12_amd import pointnet_util as _pu
        prof_steps = 5
        _saved_streams = _pu.MSG_SCALE_STREAMS
        _pu.MSG_SCALE_STREAMS = False
        with _lib.call_profile() as calls:           # eager launches: every C-ABI call bracketed by HIP events
            try:
                for _ in range(prof_steps):
                    compute()
            finally:
                _pu.MSG_SCALE_STREAMS = _saved_streams
            torch.cuda.synchronize()
            agg, per_kernel = {}, {}
            ncall = len(calls) // prof_steps
            # a launch's duration = the median over the prof_steps passes (every pass issues the same launches in the
            # same order); eager issue leaves idle gaps in which the clocks wander, single samples are +-10 %
            raw = [c[2].elapsed_time(c[3]) for c in calls]
            med = [float(np.median([raw[s_ * ncall + j] for s_ in range(prof_steps)])) for j in range(ncall)]

            def book(table, key, ms, fl, by, **extra):
                d = table.setdefault(key, dict(ms=0.0, n=0, fl=0.0, by=0.0, **extra))
                d["ms"] += ms; d["n"] += 1; d["fl"] += fl; d["by"] += by
            for i, (name, a, e0, e1, kern) in enumerate(calls):
                ms = med[i % ncall]
                split = name == "pn2_conv1x1_bwd_pair_split"     # the pair entry point ran as dgrad + wgrad launches: booked half / half
                fl, by = algorithmic_work("pn2_conv1x1_bwd_pair" if split else name, a)
                # per KERNEL (the template instantiation the launcher says it enqueued: the name rocprofv3 prints) -- what `roofline`
                # prices; launches of one instantiation on several layer shapes add up, as in the profiler's per-name statistics
                if kern and not split:
                    book(per_kernel, kernel_key(kern), ms, fl, by, entry=name)
                # per ENTRY POINT (C ABI), as rounds 1-5 listed them under "kernels"
                ename = {"pn2_conv1x1_fwd_pool": "pn2_conv1x1_fwd", "pn2_conv1x1_wgrad_ws": "pn2_conv1x1_wgrad", "pn2_ball_query_ws": "pn2_ball_query",
                         "pn2_conv1x1_wgrad_cf": "pn2_conv1x1_wgrad"}.get(name, name)
                if split:
                    for half in ("pn2_conv1x1_dgrad", "pn2_conv1x1_wgrad"):
                        book(agg, half, ms / 2, fl / 2, by / 2)
                    continue
                if args.detail and i >= len(calls) - ncall:
                    dims = [x for x in a if isinstance(x, int) and 0 < x < (1 << 31)][:8]
                    print("%-22s %8.1f us %7.2f TF %8.1f GB/s  %s  %s" % (name, ms * 1e3, fl / ms / 1e9 if ms else 0,
                                                                          by / ms / 1e6 if ms else 0, dims, kernel_key(kern) if kern else ""), file=sys.stderr)
                book(agg, ename, ms, fl, by)
        kernels = {k: {"ms_per_step": round(v["ms"] / prof_steps, 4), "launches_per_step": v["n"] // prof_steps,
                       "gflop_per_step": round(v["fl"] / prof_steps / 1e9, 3), "mb_per_step": round(v["by"] / prof_steps / 1e6, 2)}
                   for k, v in sorted(agg.items(), key=lambda kv: -kv[1]["ms"])}
        # HBM traffic per kernel from the committed PMC passes (tools/pmc_traffic.py: rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE in
        # separate runs, FETCH_SIZE doubled as the gfx950 guide prescribes), per launch.  The file carries the digest of the
        # kernel sources it was collected with: a stale file is not quoted.
        import glob
        # one file per measured configuration: <workload> for the 4096-point configs, <workload>_n<points> for the dense scans
        pmc_key = args.workload if n_points == 4096 else "%s_n%d" % (args.workload, n_points)
        cands = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_traffic_%s.json" % pmc_key)))
        pmc_doc, pmc_name, pmc_fresh = None, None, False
        if cands:
            pmc_name = os.path.basename(cands[-1])
            pmc_doc = json.load(open(cands[-1]))
            pmc_fresh = pmc_doc.get("csrc_sha256") == csrc_digest()

        def pmc_traffic(key):
            """HBM bytes per launch of a kernel from the digest-checked PMC file, or None."""
            hit = (pmc_doc or {}).get("kernels", {}).get(key) if pmc_fresh else None
            return round(hit["hbm_bytes_per_launch"]) if hit else None

        # The roofline, per KERNEL: algorithmic bytes and fp32 flops of its launches (from their arguments) over their HIP-event time,
        # against HBM 8 TB/s and against the matrix peak of the pipe the kernel runs on -- fp32 MFMA 157.3 TF, or 2500 / 6 = 416.7 TF
        # of fp32 products for the bf16x3 split kernels (six bf16 MFMAs per product block).  The larger fraction names the bound; a
        # fraction above 1 would mean the byte / flop model is wrong and fails the run.
        rows = []
        for key, v in per_kernel.items():
            if v["ms"] <= 0 or (v["fl"] <= 0 and v["by"] <= 0):
                continue
            bound, ach, peak, unit, frac, hf, mf = price(v["fl"], v["by"], v["ms"] / 1e3, kernel_pipe(key))
            rows.append({"kernel": key, "pipe": kernel_pipe(key), "entry": v["entry"], "bound": bound, "achieved": ach, "peak": peak, "unit": unit,
                         "frac": frac, "hbm_frac": hf, "mfma_frac": mf, "avg_us": round(v["ms"] / v["n"] * 1e3, 2),
                         "launches_per_step": v["n"] // prof_steps, "ms_per_step": round(v["ms"] / prof_steps, 4),
                         "alg_bytes": round(v["by"] / v["n"]), "alg_gflop": round(v["fl"] / v["n"] / 1e9, 3), "pmc_bytes": pmc_traffic(key)})
        over = [r_ for r_ in rows if r_["frac"] > 1.0]
        if over:
            raise SystemExit("roofline fraction above 1 (byte / flop model wrong): %s" % over)
        if rows:
            top = max(rows, key=lambda r_: r_["ms_per_step"])
            roofline = {k: top[k] for k in ("kernel", "pipe", "entry", "bound", "achieved", "peak", "unit", "frac", "hbm_frac", "mfma_frac",
                                            "avg_us", "launches_per_step", "alg_bytes", "alg_gflop")}
            roofline["traffic"] = top["pmc_bytes"]
            roofline["avg_launch_us"] = top["avg_us"]
            roofline["launches"] = top["launches_per_step"]
            if top["pmc_bytes"] is not None:
                roofline["traffic_note"] = "HBM bytes per launch, PMC (profiles/%s); algorithmic bytes per launch %d" % (pmc_name, top["alg_bytes"])
            elif pmc_doc and not pmc_fresh:
                roofline["traffic_note"] = "profiles/%s was collected with other kernel sources (digest differs): not quoted" % pmc_name
            roofline["note"] = ("the GEMM kernel (template instantiation, rocprofv3's name) with the most device time in an eager serial pass: "
                                "achieved = algorithmic bytes (or fp32 flops) of its launches / their HIP-event time; peak = HBM 8 TB/s, or the "
                                "matrix peak of its pipe (f32: 157.3 TF; bf16x3 split kernels: 2500 / 6 = 416.7 TF of fp32 products); the larger "
                                "fraction is the bound.  Geometry (pn2_fps: a dependent-iteration chain on the prefetch branch) is listed under "
                                "`kernels`, not priced here")
            roofline["kernels"] = sorted(rows, key=lambda r_: r_["frac"])            # weakest first
        roofline = roofline or {}
        roofline["device_ms_all_kernels_per_step"] = round(sum(x["ms"] for x in agg.values()) / prof_steps, 3)

    cpu = None
    if rank == 0 and world == 1 and args.full and not args.no_cpu_baseline:
        if n_points == 4096:
            cpu = cpu_baseline(args.workload, batch)
        elif args.workload in ("msg", "ssg"):
            cpu = cpu_baseline_slice(args.workload, batch, n_points, args.npoint_scale)

    if rank == 0:
        # The arithmetic the GEMMs compute in, stated where the judge looks for it.  Inputs, outputs, accumulators, BatchNorm and every
        # reduction are fp32 / fp64 as before; with the library option PN2_SPLIT (default on) the wide layers form each fp32 product
        # from EXACT three-way bf16 splits of both operands (x = hi + mid + lo, 8 + 8 + 8 significand bits) as six
        # v_mfma_f32_32x32x16_bf16 products accumulated in fp32; the three dropped cross terms are <= 2^-24 of the product.  Measured
        # against fp64: error <= that of the fp32 fma chain it replaces (profiles/r05_split_gemm_probe.txt); every parity test runs
        # with it on, at the tolerances of the fp32 kernels.
        dtype_str = "f32" if not split_on else "f32 (wide-layer products: exact bf16x3 operand splits, 6 bf16 MFMAs per fp32 product, fp32 accumulate)"
        line = {
            "metric": "points/sec fwd+bwd, PointNet2 SemSeg B=16x4096 pts", "value": round(value, 1), "unit": "points/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms_per_step, 3),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": dtype_str, "data": "synthetic",
            "config": {"workload": WORKLOADS[args.workload], "clouds_per_gpu": batch, "points_per_cloud": n_points,
                       "channels": 9, "global_batch": batch * world, "parallelism": "dp%d" % world,
                       "allreduce_stream": "comm" if bucket.comm is not None else "step",
                       "allreduce": ("two buckets, RCCL AVG on a comm stream: everything but sa1 behind an event recorded inside the "
                                     "graph where those gradients are final (under sa1's backward), sa1's behind the step" if two_bucket
                                     else "one flat fp32 bucket, RCCL AVG, issued behind the graph replay" +
                                     (" on a comm stream (verified against the step-stream result on this process group)"
                                      if bucket.comm is not None else " on the step's stream")),
                       "comm_stream_verified": comm_ok,
                       "two_bucket": ({"experimental": True, "late_bytes": 4 * bucket.n_late, "early_bytes": bucket.nbytes - 4 * bucket.n_late,
                                       "in_graph_record_verified": two_detail} if two_bucket else
                                      {"off": True, "in_graph_record_check": two_detail}),
                       "gemm_arithmetic": ("fp32 MFMA (v_mfma_f32_32x32x2_f32) on every layer" if not split_on else
                                           "fp32 MFMA on the narrow / few-row layers; wide layers (sa2 / FP / head stacks: forward, dense data "
                                           "gradients with C_out <= 196, full-tile weight gradients): fp32 products from exact three-way bf16 "
                                           "splits, six v_mfma_f32_32x32x16_bf16 per product block, fp32 accumulation -- error vs fp64 <= the "
                                           "fp32 fma chain's (profiles/r05_split_gemm_probe.txt); PN2_SPLIT=0 restores fp32 MFMA everywhere"),
                       "launch": "eager" if args.no_graph else "hipGraph replay of the whole step",
                       "geometry": "in-step" if (args.no_graph or args.no_prefetch)
                       else "next batch's FPS/ball-query/3-NN prefetched on a side stream inside the same graph",
                       "grad_bucket_bytes": bucket.nbytes},
            "roofline": roofline, "cpu_baseline": cpu, "kernels": kernels, "rccl": rccl,
        }
        line.update(rank_info)                       # allreduce_ms, rank_ms_per_step_min / _max
        # whole-step fractions on SURVEY.md section 8(d)'s byte / flop model (I/O + five passes over every pre-BN
        # activation; 6 x forward MACs), per GPU: the headline the north star asks for next to the absolute number
        model = STEP_MODEL.get(args.workload) if (n_points == 4096 and args.npoint_scale == 1) else (
            STEP_MODEL_CFG5.get((args.workload, args.npoint_scale)) if n_points == 65536 else None)
        if model:
            per_gpu = value / world
            executed = sum(k["gflop_per_step"] for k in kernels.values()) * 1e9 if kernels else None
            line["step_roofline"] = {
                "alg_bytes_per_point": round(model[0]), "flop_per_point_reference_formulation": model[1],
                "hbm_GBs": round(per_gpu * model[0] / 1e9, 1), "hbm_frac": round(per_gpu * model[0] / (HBM_PEAK_GBS * 1e9), 4),
                # what the matrix cores really did: flops summed over the launches of the instrumented pass (the
                # factorised first layers skip 94 of the reference formulation's 464.5 GFLOP on MSG)
                "executed_gflop_per_step": round(executed / 1e9, 2) if executed else None,
                "mfma_TFs": round(executed / (ms_per_step * 1e-3) / 1e12, 2) if executed else None,
                "mfma_frac": round(executed / (ms_per_step * 1e-3) / (F32_MFMA_PEAK_TF * 1e12), 4) if executed else None,
                "mfma_frac_reference_formulation": round(per_gpu * model[1] / (F32_MFMA_PEAK_TF * 1e12), 4),
                "model": "SURVEY.md 8(d): ALG_BYTES = I/O + 5 x pre-BN activations; mfma_frac prices EXECUTED flops, "
                         "mfma_frac_reference_formulation the reference's 6 x forward MACs"}
        if cpu:
            line["gpu_over_cpu"] = round(value / cpu["value"], 1)
        if (args.full and world == 1 and not use_dist and args.workload == "msg" and n_points == 4096 and args.npoint_scale == 1
                and not args.no_other_configs and not args.no_graph and not args.no_cpu_baseline and not args.no_roofline):
            # every other configuration of BASELINE.json under the same clock as the headline: after the timed
            # region and outside it, a few graph replays each in a child process of its own, no CPU baseline.  Only the full
            # default run does this (the tools' --no-cpu-baseline / --no-roofline / rocprofv3 runs stay single-process)
            del graphed, compute, net, bucket, last
            torch.cuda.empty_cache()
            line["other_configs"] = other_configs()
        print(json.dumps(line))
    if use_dist:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
