"""Throughput bench of the north-star path: res15 eval forward over synthetic
[B,101,40] fp32 MFCC maps resident in HBM, on the gfx950 kernels.

    python bench.py [--gpus N --steps K --warmup W --batch B]
    torchrun --nproc-per-node N bench.py --gpus N ...   (one rank per GPU)

``--gpus N`` without a torchrun environment: this process never touches the GPU;
it starts N rank processes (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* set, one
GPU each, RCCL) and exits with their status.  Only rank 0 prints.

One step = one forward of B clips per GPU (weak scaling: per-GPU batch fixed;
the batch shards across ranks with no collective on the data path).  Prints ONE
JSON line on rank 0 (see DESIGN.md "Measurement").  A plain run measures only
the headline (res15, f16x2: the fastest mode that meets the 1e-4 logit bar on
res15): set-up, warm-up, the timed steps, the result line.  ``--full`` adds
everything else to the line: the sample parity against the float64 oracle, the
f16x2 admission report on the range fixtures, the other res15 precision modes,
the BASELINE.json configs C2 (cnn-trad-pool2 fp32 + bf16x3), C3 (res8 bf16) and
C5 (res26-narrow training, DP over RCCL), each with its roofline, and the CPU
baseline.  ``--dump-outputs DIR`` writes what the last timed step returned
(DIR/logits.npy, float32; DIR/loss.npy under --train) so that two builds can be
compared output for output: the inputs are seeded and identical from run to run.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

METRIC = "1s-clips/sec (whole node) + top-1 acc, res15 12-label Speech Commands"
FP32_MFMA_PEAK_TFLOPS = 157.3   # MI355X_MICROARCH.md: v_mfma_f32_*_f32 dense peak (= FP32 vector peak)
HBM_PEAK_GBS = 8000.0
BF16_MFMA_PEAK_TFLOPS = 2500.0  # dense bf16 MFMA (no sparsity)
# MFMA peak per precision mode in ALGORITHMIC flop: bf16x3 spends 3 bf16 products per MAC
# (f16x2: fp16 MFMA, same dense peak as bf16, 2 products per MAC)
MODE_PEAK = {"f32": FP32_MFMA_PEAK_TFLOPS, "bf16x3": BF16_MFMA_PEAK_TFLOPS / 3, "bf16": BF16_MFMA_PEAK_TFLOPS,
             "f16x2": BF16_MFMA_PEAK_TFLOPS / 2}
WORKLOADS = {
    "res15": "res15 eval forward (SpeechResModel, 13 dilated 3x3 res layers, 45 maps, 12 labels)",
    "res8": "res8 eval forward (SpeechResModel, avg-pool 4x3, 6 res layers, 45 maps, 12 labels)",
    "cnn-trad-pool2": "cnn-trad-pool2 eval forward (SpeechModel, conv 20x8 + maxpool 2x2 + conv 10x4 + linear, 4 labels)",
}
PREC_NOTES = {
    "bf16x3": "fp32 values carried as bf16 (hi, lo) pairs; products hi*hi + hi*lo + lo*hi on bf16 MFMA, fp32 "
              "accumulation; meets the fp32 1e-4 logit parity bar (tests/test_gpu_bf16x3.py)",
    "f32": "IEEE fp32 on v_mfma_f32_16x16x4_f32; 1e-4 logit parity",
    "bf16": "bf16 activations/weights, fp32 accumulation; top-1 parity only (reduced precision vs the fp32 "
            "reference), so never the headline",
    "f16x2": "activations as fp16 (RNE) under per-clip power-of-two scales (fp16's range follows the clip), "
             "weights (input BN folded, per-layer power-of-two exponents) as fp16 (hi, lo), products w_hi*x + "
             "w_lo*x on fp16 MFMA, fp32 accumulation; meets the fp32 1e-4 logit parity bar on res15 (goldens, "
             "calibrated random cases and reference range fixtures, tests/test_gpu_f16x2.py, test_gpu_range.py); "
             "the default 'auto' policy takes it only where that holds (honk_res_select_precision + a measured "
             "probe), bf16x3 elsewhere",
}


def parse(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=5)
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--batch", type=int, default=None,
                   help="clips per GPU per step (default: res* 131072 = C4's 1M over 8 GPUs; cnn* 65536 = C2)")
    p.add_argument("--model", default="res15")
    p.add_argument("--cpu-seconds", type=float, default=12.0)
    p.add_argument("--no-cpu-baseline", action="store_true")
    p.add_argument("--precision", default=None, choices=["auto", "f16x2", "bf16x3", "f32", "bf16"],
                   help="eval arithmetic: auto (default: what the reference's unchanged callers get -- the fastest "
                        "mode holding 1e-4 for the model, f16x2 on res15, bf16x3 on cnn), f16x2 (fp16 activations, "
                        "fp16 hi/lo weights, 2 fp16 MFMA products; 1e-4 parity on res15), bf16x3 (fp32 values as "
                        "bf16 hi/lo pairs, 3 bf16 MFMA products, fp32 accumulation; 1e-4 parity), f32 (fp32 MFMA; "
                        "1e-4 parity) or bf16 (res only; top-1 parity)")
    p.add_argument("--full", action="store_true",
                   help="beside the headline: sample parity against the float64 oracle, the f16x2 admission report, "
                        "the other precision modes, C2, C3, C5 and the CPU baseline (trimmed by --no-alt, "
                        "--no-configs, --no-cpu-baseline); without it only the headline is measured")
    p.add_argument("--dump-outputs", metavar="DIR", default=None,
                   help="after the timed steps write what the last of them returned as DIR/<name>.npy (float32; "
                        "logits, or loss under --train; a fixed seeded sample of rows past 64 MB)")
    p.add_argument("--no-alt", action="store_true",
                   help="with --full: skip the extra measurements (other precision modes, C2, C3, C5)")
    p.add_argument("--no-configs", action="store_true",
                   help="with --full: skip C2/C3/C5 (keep the other res precision modes): the rocprof passes of "
                        "tools/profile.sh")
    p.add_argument("--e2e", action="store_true",
                   help="serving pipeline: int16-scaled PCM [B,16000] in HBM -> GPU MFCC -> model -> logits")
    p.add_argument("--train", action="store_true",
                   help="only C5: data-parallel training step (fwd+bwd, one RCCL all-reduce, fused SGD)")
    return p.parse_args(argv)


def log(msg):
    """Progress on stderr (stdout carries exactly one JSON line)."""
    print(f"[bench r{os.environ.get('RANK', '0')}] {msg}", file=sys.stderr, flush=True)


# ---------------------------------------------------------------------------------------------
# --gpus N launcher: the parent never initialises HIP
# ---------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def rank_envs(n, port, base=None):
    """Environment of each rank process for a single-node N-GPU run (torchrun's variables)."""
    base = dict(os.environ if base is None else base)
    envs = []
    for r in range(n):
        e = dict(base)
        e.update(RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                 GROUP_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        envs.append(e)
    return envs


def _route(stream, is_rank0):
    """Forward a rank's stdout: rank 0's JSON result line to our stdout, everything
    else (library chatter such as gloo's connection lines) to stderr."""
    for line in iter(stream.readline, ""):
        if is_rank0 and line.lstrip().startswith("{"):
            sys.stdout.write(line)
            sys.stdout.flush()
        else:
            sys.stderr.write(line)
            sys.stderr.flush()
    stream.close()


KFD_TOPOLOGY = "/sys/class/kfd/kfd/topology/nodes"


def count_gpus_sysfs(root=None, env=None):
    """Visible GPUs counted WITHOUT the HIP runtime: KFD topology nodes whose
    properties carry a non-zero gfx_target_version (CPU nodes carry 0), capped by
    the visibility lists ROCR_VISIBLE_DEVICES / HIP_VISIBLE_DEVICES /
    CUDA_VISIBLE_DEVICES.  None when the topology is unreadable (the ranks then
    check LOCAL_RANK against their own device count)."""
    root = root or os.environ.get("HONK_KFD_TOPOLOGY", KFD_TOPOLOGY)
    env = os.environ if env is None else env
    try:
        nodes = os.listdir(root)
    except OSError:
        return None
    n = 0
    for node in nodes:
        try:
            with open(os.path.join(root, node, "properties")) as f:
                props = dict(ln.split(None, 1) for ln in f if len(ln.split(None, 1)) == 2)
        except OSError:
            continue
        try:
            if int(props.get("gfx_target_version", "0").strip()) != 0:
                n += 1
        except ValueError:
            continue
    for var in ("ROCR_VISIBLE_DEVICES", "HIP_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"):
        v = env.get(var)
        if v is not None:
            n = min(n, len([t for t in v.split(",") if t.strip()]))
    return n


def spawn_ranks(n, argv, script=None):
    """Start n rank processes of this script and wait for them; returns the exit status.

    A rank that fails ends the others (they would otherwise wait in a collective).
    This process never initialises HIP (no torch.cuda call at all): the GPUs are
    counted from the KFD topology in sysfs, and each rank also checks its
    LOCAL_RANK against its own device count (rank_main)."""
    import threading
    if not os.environ.get("HONK_BENCH_ONE_GPU"):
        have = count_gpus_sysfs()
        if have is not None and have < n:
            log(f"--gpus {n} but only {have} visible GPU(s)")
            return 2
    script = script or os.path.abspath(__file__)
    procs, pumps = [], []
    for r, e in enumerate(rank_envs(n, _free_port())):
        p = subprocess.Popen([sys.executable, "-u", script] + list(argv), env=e, stdout=subprocess.PIPE, text=True)
        t = threading.Thread(target=_route, args=(p.stdout, r == 0), daemon=True)
        t.start()
        procs.append(p)
        pumps.append(t)
    rc = 0
    alive = list(procs)
    while alive:
        for p in list(alive):
            r = p.poll()
            if r is None:
                continue
            alive.remove(p)
            if r != 0 and rc == 0:
                rc = r if r > 0 else 128 - r
                for q in alive:
                    q.terminate()
        time.sleep(0.1)
    for t in pumps:
        t.join(timeout=10)
    return rc


# ---------------------------------------------------------------------------------------------
# CPU baseline
# ---------------------------------------------------------------------------------------------
def cpu_share():
    """Host threads this process may use: the CPU affinity mask, capped by a cgroup
    cpu.max quota and by OMP_NUM_THREADS when set (16 on the GPU pool, whose
    os.cpu_count() shows the whole machine)."""
    try:
        n = len(os.sched_getaffinity(0))
    except (AttributeError, OSError):  # pragma: no cover
        n = os.cpu_count() or 1
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:
            q, per = f.read().split()[:2]
        if q != "max":
            n = min(n, max(1, int(float(q) / float(per))))
    except (OSError, ValueError):
        pass
    omp = int(os.environ.get("OMP_NUM_THREADS") or 0)
    if omp > 0:
        n = min(n, omp)
    return max(1, n)


def cpu_baseline(cfg, seconds):
    """The reference's CPU path restated (oracle/ref_torch.py: stock torch fp32 eval
    forward, what utils/train.py --no_cuda runs) on the host cores: bounded sample,
    batches as SURVEY.md §8(d): 64 clips for res15, else 256."""
    from oracle import ref_numpy as orc
    from oracle import ref_torch
    cores = cpu_share()
    torch.set_num_threads(cores)
    params = ref_torch.tensors(orc.make_params(cfg, 0))
    rng = np.random.Generator(np.random.PCG64(1))
    per = 64 if int(cfg.get("n_layers", 0)) > 8 else 256
    x = torch.from_numpy(rng.standard_normal((per, 101, 40)).astype(np.float32))
    ref_torch.forward(params, cfg, x[:2])  # warm-up
    ref_torch.forward(params, cfg, x)
    n = 0
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        ref_torch.forward(params, cfg, x)
        n += per
    dt = time.perf_counter() - t0
    model_name = "unknown"
    try:
        with open("/proc/cpuinfo") as f:
            model_name = next((ln.split(":", 1)[1].strip() for ln in f if ln.startswith("model name")), model_name)
    except OSError:  # pragma: no cover
        pass
    return {"value": n / dt, "unit": "clips/s", "cores": int(cores), "kind": "port",
            "sample": f"{n} clips of {cfg_name(cfg)} in {dt:.1f} s (oracle/ref_torch.py: torch {torch.__version__} "
                      f"CPU fp32 eval forward, batches of {per}, {cores} threads)",
            "cpu_model": model_name, "os_cpu_count": os.cpu_count(),
            "threads_source": "sched_getaffinity / cgroup cpu.max / OMP_NUM_THREADS"}


def cfg_name(cfg):
    if "n_layers" not in cfg:
        return "cnn"
    return (f"res (n_layers {cfg['n_layers']}, {cfg['n_feature_maps']} maps"
            f"{', dilated' if cfg.get('use_dilation') else ''})")


# ---------------------------------------------------------------------------------------------
# rooflines
# ---------------------------------------------------------------------------------------------
def load_traffic(kernel, clips_per_launch, model):
    """HBM bytes per launch of `kernel` from a committed rocprofv3 PMC pass
    (profiles/pmc_<kernel>.json, written by tools/pmc_summary.py), or None when no
    pass was taken for that kernel at this launch size."""
    for fn in (f"pmc_{kernel}_{model}.json", f"pmc_{kernel}.json"):
        p = os.path.join(REPO, "profiles", fn)
        if not os.path.exists(p):
            continue
        try:
            with open(p) as f:
                d = json.load(f)
        except Exception:
            continue
        if d.get("batch_clips_per_launch") == clips_per_launch and d.get("model") == model:
            return d.get("hbm_bytes_per_launch", d.get("hbm_bytes_per_step"))
    return None


def _res_geometry(cfg):
    """(H, W, n_layers, CP) of a res config's block layers (model.py:87-98)."""
    ph, pw = tuple(cfg.get("res_pool", (1, 1)))
    C = int(cfg["n_feature_maps"])
    return 101 // ph, 40 // pw, int(cfg["n_layers"]), 16 * ((C + 15) // 16)


def res_roofline(prec, cfg, kms, nl, kfl, B, model, plan, steps=None):
    """Roofline of the res block convs (the dilated 3x3 layers) for a precision mode.

    MFMA-bound: achieved = ALGORITHMIC flop (2 x 9 x C^2 x H x W per
    clip-layer, no padding, one product per MAC) over all timed block-kernel
    launches / their summed time (HIP events on the launch stream); peak = the MFMA
    peak of the mode in algorithmic flop (fp32 157.3 TF; bf16x3 = bf16 2.5 PF / 3
    products; bf16 2.5 PF).  `plan` = the launches of one chunk's forward
    (honk_res_launch_plan): block16p_kernel launches run a fused odd/even layer pair.
    Beside it: the activation bytes the schedule moves per clip (a fused pair reads
    its input once and the residual once and writes once; a single layer reads its
    input [and the residual] and writes its output unless it is the last) as an
    HBM rate, and the dominant kernel's PMC-measured HBM traffic per launch."""
    H, W, L, CP = _res_geometry(cfg)
    ach = kfl / (kms * 1e-3) / 1e12 if nl and kms else None
    peak = MODE_PEAK[prec]
    chunk_fwds = nl / max(len(plan), 1)
    # clips per chunk (the library's chunk_clips: 4096, 8192 for pooled maps): the timed
    # clips over the chunk forwards the timed launches make up
    clips = int(round(B * steps / chunk_fwds)) if steps and chunk_fwds else min(B, 4096)
    if prec == "f32":
        act = H * W * CP * 4
        per_clip = sum(act * (1 + (1 if i % 2 == 0 else 0) + (1 if i < L else 0)) for i in range(1, L + 1))
        dom, traffic = "block_kernel", load_traffic("block_kernel", clips, model)
        kname = "honk::res::block_kernel (dilated 3x3 conv, fp32 MFMA)"
    else:
        sp = 2 if prec == "bf16x3" else 1
        tag = "f16" if prec == "f16x2" else f"sp{sp}"
        act = H * W * CP * 2 * sp
        per_clip, layer = 0, 1
        for k in plan:
            if k in ("block16p_kernel", "block16k_kernel"):
                per_clip += 3 * act
                layer += 2
            elif k == "block16n_kernel":  # the whole stack: the conv0 output read once
                per_clip += act
                layer += L
            else:
                per_clip += act * (1 + (1 if layer % 2 == 0 else 0) + (1 if layer < L else 0))
                layer += 1
        dom = max(set(plan), key=plan.count)
        traffic = load_traffic(f"{dom}_{tag}", clips, model)
        what = {"block16p_kernel": "fused odd + even layer pair", "block16w_kernel": "weight-stationary layer",
                "block16k_kernel": "fused odd + even layer pair, K split over two waves per SIMD",
                "block16l_kernel": "last layer on the pair's streaming machinery, fused channel sums",
                "block16r_kernel": "row-band layer",
                "block16n_kernel": "every block layer of a clip, activations resident in LDS"}
        kname = (" + ".join(f"honk::res::{k}<..., {tag}> x{plan.count(k)} ({what[k]})"
                            for k in sorted(set(plan), key=plan.index))
                 + " per chunk: dilated 3x3 convs, "
                 + {"bf16x3": "bf16 MFMA, 3 products", "bf16": "bf16 MFMA", "f16x2": "fp16 MFMA, 2 products"}[prec])
    secs = kms * 1e-3
    bw = per_clip * clips * chunk_fwds / secs / 1e9 if nl and secs else None
    out = {"bound": "mfma", "kernel": kname,
           "achieved": round(ach, 2) if ach else None, "peak": round(peak, 1), "unit": "TFLOP/s",
           "frac": round(ach / peak, 4) if ach else None,
           "traffic": traffic, "traffic_kernel": dom,
           "launches": nl, "launch_plan_per_chunk": _plan_str(plan), "clips_per_chunk": clips,
           "avg_ms_per_layer": round(kms / max(chunk_fwds * L, 1), 4),
           "avg_ms_per_launch": {k: None for k in ()},
           "flop_per_layer": kfl / max(chunk_fwds * L, 1),
           "flop_def": "algorithmic: 2*9*C^2*H*W per clip-layer (SURVEY §8(d)), no channel/tile padding",
           "hbm": {"activation_bytes_per_clip": per_clip,
                   "achieved_GBs": round(bw, 1) if bw else None, "peak_GBs": HBM_PEAK_GBS,
                   "frac": round(bw / HBM_PEAK_GBS, 4) if bw else None}}
    del out["avg_ms_per_launch"]
    if prec in ("bf16x3", "f16x2") and ach:
        out["frac_of_raw_bf16_peak"] = round(ach / BF16_MFMA_PEAK_TFLOPS, 4)
    return out


MFCC_SCALE = [20.0] + [8.0 / (1 + k) for k in range(1, 40)]


def mfcc_like(B, dev, gen):
    """SURVEY §8(d)'s MFCC-like synthetic clips, made in HBM: c0 ~ N(-30, 20^2),
    c_k ~ N(0, (8 / (1 + k))^2) (the golden fixtures' "mfcc" distribution)."""
    x = torch.randn(B, 101, 40, device=dev, generator=gen) * torch.tensor(MFCC_SCALE, device=dev)
    x[:, :, 0] -= 30.0
    return x


def bench_model(name, dev):
    """The bench's model: the reference constructor's random init (torch.manual_seed(0));
    res models get BatchNorm running statistics calibrated on MFCC-like clips
    (oracle.ref_numpy.calibrate_bn: the float64 batch statistics plus a 0.5-std mean
    shift, as the golden fixtures), so every layer runs at unit scale with non-zero channel
    means -- the parity sample then exercises the whole conv stack (default statistics,
    mean 0 / var 1, leave the fp16 rounding nearly invisible)."""
    from honk_amd import model as hm
    from oracle import ref_numpy as orc
    cfg = dict(hm.find_config(name))
    torch.manual_seed(0)
    model = hm.find_model(name)(cfg)
    if name.startswith("res"):
        params = {k: v.detach().numpy() for k, v in model.state_dict().items()}
        rng = np.random.Generator(np.random.PCG64(7))
        xc = rng.standard_normal((2, 101, 40)) * np.array(MFCC_SCALE)
        xc[:, :, 0] -= 30.0
        params = orc.calibrate_bn(params, cfg, xc.astype(np.float32), seed=7)
        with torch.no_grad():
            for i in range(1, int(cfg["n_layers"]) + 1):
                bn = getattr(model, f"bn{i}")
                bn.running_mean.copy_(torch.from_numpy(params[f"bn{i}.running_mean"]))
                bn.running_var.copy_(torch.from_numpy(params[f"bn{i}.running_var"]))
    return model.eval().to(dev)


def admission_report(dev):
    """What ``auto`` does on the reference-written range fixtures (outside the timed
    region): the realistic-scale res15-speech case (speech-like PCM -> MFCC, c0 about
    -20..-150, BN calibrated on it) and an out-of-distribution batch (range_res15-ood:
    inputs x 3000) fed to its unit-calibrated model after a calibrated batch -- the mode
    picked, the clips the per-clip f16x2 admission re-ran in bf16x3, and the error against
    the reference's logits (tests/golden/make_range_golden.py)."""
    sys.path.insert(0, os.path.join(REPO, "tests"))
    try:
        from golden_util import load_fixture, load_range_fixture
    finally:
        sys.path.pop(0)
    from honk_amd import model as hm
    out = {}

    def one(m, x, want):
        with torch.no_grad():
            got = m(torch.as_tensor(x).to(dev)).cpu().numpy()
        err = np.abs(got - want)
        return {"mode": m.honk_last_precision, "rerun_clips": m.honk_last_rerun, "clips": len(x),
                "max_abs_err": float(err.max()),
                "max_err_over_bar": float((err / (1e-4 * np.maximum(1, np.abs(want).max(1, keepdims=True)))).max())}

    def module(cfg, params, name):
        m = hm.find_model(name)(cfg)
        m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in params.items()})
        return m.eval().to(dev)

    cfg, params, x, logits, name = load_range_fixture("res15-speech")
    out["res15_speech_realistic"] = one(module(cfg, params, name), x, logits)
    cfg, params, x, logits, meta = load_fixture("res15-b3-mfcc")
    m = module(cfg, params, "res15")
    out["res15_calibrated_then_ood"] = [one(m, x, logits)]
    _, _, x, logits, _ = load_range_fixture("res15-ood")
    out["res15_calibrated_then_ood"].append(one(m, x, logits))
    out["note"] = ("auto = the reference callers' default; max_err_over_bar = |err| / (1e-4 max(1, |logit|)) "
                   "per clip; the ood batch's clips leave the model's calibration (|z| > 8) and re-run in bf16x3")
    return out


def _plan_str(plan):
    return " + ".join(f"{k} x{plan.count(k)}" for k in sorted(set(plan), key=plan.index))


def _sample_parity(model, cfg, x, out, orc, B):
    idx = list(range(0, B, max(1, B // 32)))[:32]
    ref = orc.forward({k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}, cfg,
                      x[idx].cpu().numpy())
    got = out[idx].cpu().numpy()
    return {"top1_agreement_vs_oracle": float(np.mean(ref.argmax(1) == got.argmax(1))),
            "max_abs_logit_err_vs_oracle_f64": float(np.abs(ref - got).max()),
            "sample_clips": len(idx)}


DUMP_MAX_BYTES = 64 << 20


def dump_outputs(dirname, arrays, rank=0, world=1):
    """--dump-outputs: what the last timed step returned, as DIR/<name>.npy in float32
    (DIR/<name>_rank<r>.npy per rank when world > 1).  The whole dump stays within
    DUMP_MAX_BYTES: an array past its share is cut to a fixed, seeded sample of its
    rows (in index order)."""
    os.makedirs(dirname, exist_ok=True)
    share = DUMP_MAX_BYTES // max(1, world * len(arrays))
    for name, t in arrays.items():
        a = np.ascontiguousarray(t.detach().to(torch.float32).cpu().numpy())
        if a.nbytes > share and a.ndim >= 1 and len(a) > 1:
            keep = max(1, share // max(1, a.nbytes // len(a)))
            idx = np.sort(np.random.Generator(np.random.PCG64(2024)).choice(len(a), size=keep, replace=False))
            a = a[idx]
        np.save(os.path.join(dirname, name + (f"_rank{rank}" if world > 1 else "") + ".npy"), a)


def modes_summary(res, model):
    """Every measured mode and config as {value, dtype, frac}: printed as the line's last
    key, so a driver that keeps only the tail of stdout still sees every number."""
    def one(d, dtype=None):
        r = d.get("roofline") or {}
        return {"value": d.get("value"), "dtype": dtype or d.get("dtype"), "frac": r.get("frac")}
    out = {f"{model}_{res['dtype']} (headline)": one(res)}
    for k, v in res.items():
        if k.endswith("_mode") and isinstance(v, dict) and "value" in v:
            out[f"{model}_{v['dtype']}"] = one(v)
    c2 = res.get("c2_cnn_trad_pool2")
    if c2:
        for p in ("f32", "bf16x3"):
            if f"{p}_mode" in c2:
                out[f"c2_cnn-trad-pool2_{p}"] = one(c2[f"{p}_mode"])
    for k in ("c3_res8_bf16", "c5_res26_narrow_train"):
        if k in res:
            out[k] = one(res[k])
    if "cpu_baseline" in res:
        out["cpu_baseline"] = {"value": round(res["cpu_baseline"]["value"], 1),
                               "cores": res["cpu_baseline"]["cores"]}
    return out


class Ctx:
    """What every measurement needs: device, ranks, barrier, native handle."""

    def __init__(self, dev, rank, world, dist):
        from honk_amd import _native
        from honk_amd import distributed as hd
        self.dev, self.rank, self.world, self.dist = dev, rank, world, dist
        self.native, self.hd = _native, hd

    def barrier(self):
        if self.dist:
            import torch.distributed as tdist
            tdist.barrier()

    def timed(self, fn, x, steps, warmup):
        """Run warmup + steps of fn(x) between barriers; returns (max-over-ranks seconds,
        per-rank seconds, last output, (kernel ms, launches, flop))."""
        with torch.no_grad():
            for _ in range(warmup):
                fn(x)
            torch.cuda.synchronize()
            self.barrier()
            torch.cuda.synchronize()
            self.native.timing_enable(True)
            t0 = time.perf_counter()
            for _ in range(steps):
                out = fn(x)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            self.barrier()
            k = self.native.timing_read()
            self.native.timing_enable(False)
        per = self.hd.gather_scalar(t1 - t0, device=self.dev)
        return max(per), per, out, k


def measure_res(ctx, args, name, prec, B, x=None, model=None):
    """A res model's eval forward of B clips per GPU in one precision mode."""
    from honk_amd import model as hm
    from oracle import ref_numpy as orc
    cfg = dict(hm.find_config(name))
    if model is None:
        model = bench_model(name, ctx.dev)
    if x is None:
        g = torch.Generator(device=ctx.dev).manual_seed(1234 + ctx.rank)
        x = mfcc_like(B, ctx.dev, g)
    keep = (model.honk_precision, model.honk_reroute)
    # the named mode's own kernels (the policy's choice is the headline's business)
    model.honk_precision, model.honk_reroute = prec, False
    el, per, out, (kms, nl, kfl) = ctx.timed(model, x, args.steps, max(1, args.warmup))
    plan = ctx.native.res_launch_plan(model._desc(101, 40, prec), B)
    model.honk_precision, model.honk_reroute = keep
    return {"value": round(ctx.world * B * args.steps / el, 1), "unit": "clips/s", "dtype": prec,
            "ms_per_step": round(el / args.steps * 1e3, 3),
            "per_rank_clips_s": [round(B * args.steps / t, 1) for t in per],
            "roofline": res_roofline(prec, cfg, kms, nl, kfl, B, name, plan, args.steps),
            "parity": _sample_parity(model, cfg, x, out, orc, B),
            "note": PREC_NOTES[prec]}


def measure_c2(ctx, args):
    """Config C2 (BASELINE.json configs[1]): cnn-trad-pool2 eval forward, 65,536
    clips per GPU, in fp32 (the config as named) and bf16x3 (1e-4 parity).
    Roofline: algorithmic conv FLOP per launch over the conv kernels' mean launch
    time (HIP events on the launch stream), vs the fp32 MFMA peak (resp. bf16 peak / 3)."""
    from honk_amd import model as hm
    from oracle import ref_numpy as orc
    name = "cnn-trad-pool2"
    cfg = dict(hm.find_config(name))
    model = bench_model(name, ctx.dev)
    B = 65536
    g = torch.Generator(device=ctx.dev).manual_seed(4321 + ctx.rank)
    x = mfcc_like(B, ctx.dev, g)
    out = {"workload": "cnn-trad-pool2 eval forward (config C2), 65,536 clips per GPU", "per_gpu_batch": B}
    for prec in ("f32", "bf16x3"):
        model.honk_precision = prec
        el, per, y, (kms, nl, kfl) = ctx.timed(model, x, args.steps, max(1, args.warmup))
        peak = MODE_PEAK[prec]
        ach = (kfl / max(nl, 1)) / (kms / max(nl, 1) * 1e-3) / 1e12 if nl else None
        out[f"{prec}_mode"] = {
            "value": round(ctx.world * B * args.steps / el, 1), "unit": "clips/s", "dtype": prec,
            "ms_per_step": round(el / args.steps * 1e3, 3),
            "per_rank_clips_s": [round(B * args.steps / t, 1) for t in per],
            "roofline": {"bound": "mfma",
                         "kernel": ("honk::cnn::conv1x3_kernel + conv2x3_kernel (bf16x3 convs, 3 bf16 MFMA "
                                    "products per MAC; peak = bf16 peak / 3)" if prec == "bf16x3" else
                                    "honk::cnn::conv1f_kernel + conv2f_kernel (fused conv1+ReLU+max-pool and whole-clip conv2, "
                                    "fp32 MFMA 16x16x4)"),
                         "achieved": round(ach, 2) if ach else None, "peak": round(peak, 1), "unit": "TFLOP/s",
                         "frac": round(ach / peak, 4) if ach else None, "launches": nl,
                         "avg_launch_ms": round(kms / max(nl, 1), 4), "flop_per_launch": kfl / max(nl, 1),
                         "traffic": load_traffic(f"c2_{prec}_convs", B, name),
                         "traffic_def": "PMC HBM bytes per conv launch (conv1 and conv2 launches pooled, "
                                        "profiles/pmc_c2_<mode>_convs_cnn-trad-pool2.json)"},
            "parity": _sample_parity(model, cfg, x, y, orc, B),
            "note": PREC_NOTES.get(prec, "")}
    del x
    return out


def train_flops_per_clip(cfg):
    """Algorithmic training FLOP per clip: forward + input grad (every layer but conv0)
    + weight grad, each 2 x MACs (~3x forward - conv0 dgrad)."""
    from oracle import ref_numpy as orc
    fwd = orc.flops_per_clip(cfg)
    conv0 = 2 * 101 * 40 * int(cfg["n_feature_maps"]) * 9
    return 3 * fwd - conv0


def measure_train(ctx, args, name="res26-narrow", B=None, dump=None):
    """C5: res26-narrow train step per rank (fwd+bwd on device, flat-bucket all-reduce
    over RCCL when world > 1, fused SGD).  Roofline: algorithmic training FLOP per
    step / step time vs the fp32 peak (the native training convs are fp32)."""
    from honk_amd import model as hm
    from honk_amd.head_train import CrossEntropyLoss
    from honk_amd.optim import FlatParams, FlatSGD
    hd = ctx.hd
    B = B or 4096
    cfg = dict(hm.find_config(name))
    torch.manual_seed(0)
    model = hm.find_model(name)(cfg).to(ctx.dev).train()
    hd.broadcast_module(model)
    flat = FlatParams(model)
    fbuf = hd.FlatBuffers(model)      # BN running stats: one broadcast per step
    reducer = hd.GradAllReduce(flat)  # one all-reduce per step, started by backward's last gradient
    opt = FlatSGD(flat, lr=0.1, momentum=0.9, weight_decay=1e-5)
    crit = CrossEntropyLoss()
    g = torch.Generator(device=ctx.dev).manual_seed(99 + ctx.rank)
    x = torch.randn(B, 101, 40, device=ctx.dev, generator=g)
    y = torch.randint(0, cfg["n_labels"], (B,), device=ctx.dev, generator=g)
    from honk_amd.head_train import check_labels
    check_labels(y, cfg["n_labels"])  # once: the batch is fixed

    def step():
        opt.zero_grad()
        hd.broadcast_buffers(fbuf)
        loss = crit(model(x), y, labels_checked=True)
        loss.backward()
        opt.step(grad_scale=reducer.wait())
        return loss

    # parity of the timed workload itself (outside the timed region): the first step's
    # training-mode loss on the native kernels vs the same model on stock PyTorch ops
    # (MIOpen convs, ATen BatchNorm / mean / Linear / cross-entropy), same weights and batch.
    # HONK_BENCH_TRAIN_PARITY=0 skips it (the PMC passes of tools/profile_configs.sh: only
    # the step's own kernels in the counters)
    import copy
    l_nat = l_ref = None
    if os.environ.get("HONK_BENCH_TRAIN_PARITY", "1") != "0":
        with torch.no_grad():
            m_nat, m_ref = copy.deepcopy(model), copy.deepcopy(model)
            m_ref.honk_native_train = False
            l_nat = float(crit(m_nat(x), y))
            l_ref = float(torch.nn.functional.cross_entropy(m_ref(x), y))
            del m_nat, m_ref
        torch.cuda.empty_cache()

    for _ in range(max(1, args.warmup)):
        step()
    torch.cuda.synchronize()
    ctx.barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        loss = step()
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    ctx.barrier()
    reducer.remove()  # no gradient hooks outlive the timed steps
    if dump:
        dump_outputs(dump, {"loss": loss.detach().reshape(1)}, ctx.rank, ctx.world)
    per = hd.gather_scalar(t1 - t0, device=ctx.dev)
    el = max(per)
    fl = train_flops_per_clip(cfg)
    ach = B * args.steps * fl / el / 1e12
    return {
        "metric": "train clips/sec (whole node), res26-narrow fwd+bwd+SGD, DP over RCCL (config C5)",
        "value": round(ctx.world * B * args.steps / el, 1), "unit": "clips/s", "dtype": "f32",
        "ms_per_step": round(el / args.steps * 1e3, 3),
        "per_rank_clips_s": [round(B * args.steps / t, 1) for t in per],
        "config": {"workload": f"{name} training step (train-mode BN batch stats, CE loss, SGD m=0.9, wd 1e-5)",
                   "per_gpu_batch": B, "global_batch": ctx.world * B,
                   "parallelism": f"dp{ctx.world}: per step one broadcast of the BN-stat bucket and one all-reduce "
                                  f"of the flat fp32 grad bucket ({flat.numel} params)"},
        "final_loss": float(loss.item()),
        "parity": {"step0_loss_native": l_nat, "step0_loss_pytorch_fp32": l_ref,
                   "abs_diff": abs(l_nat - l_ref) if l_nat is not None else None,
                   "note": "first step's train-mode loss, native kernels vs stock PyTorch ops on the same weights "
                           "and 4096-clip batch (the gradients are pinned by tests/test_train_golden.py)"},
        "roofline": {"bound": "mfma", "kernel": "whole training step (per-GPU)",
                     "achieved": round(ach, 2), "peak": FP32_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
                     "frac": round(ach / FP32_MFMA_PEAK_TFLOPS, 4),
                     "traffic": load_traffic("train_step", B, name),
                     "traffic_def": "PMC HBM bytes of every kernel of one training step "
                                    "(profiles/pmc_train_step_<model>.json)",
                     "flop_per_clip": fl,
                     "flop_def": "2 x (forward + input-grad + weight-grad MACs), conv0 has no input grad"},
        "note": "native kernels: the stem (conv0 + relu + avg-pool, conv0 weight grad), the block convs' "
                "forward / input grad / weight grad on fp32 MFMA, each block's relu + residual + train-mode "
                "BatchNorm fwd/bwd fused, the spatial mean, the Linear and the cross-entropy loss "
                "(honk_amd/head_train.py), fused SGD over the flat all-reduced bucket"}


def rank_main(args):
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    dist = world > 1
    if not os.environ.get("HONK_BENCH_ONE_GPU") and local >= torch.cuda.device_count():
        log(f"LOCAL_RANK {local} but only {torch.cuda.device_count()} visible GPU(s)")
        sys.exit(2)
    if dist:
        import torch.distributed as tdist
        # rehearsal knobs for a 1-GPU box (never set by the driver): HONK_BENCH_BACKEND=gloo
        # and HONK_BENCH_ONE_GPU=1 run N ranks on cuda:0 over gloo; the real N-GPU run is RCCL
        if os.environ.get("HONK_BENCH_ONE_GPU"):
            local = 0
        backend = os.environ.get("HONK_BENCH_BACKEND", "nccl")
        torch.cuda.set_device(local)
        if backend == "nccl":
            tdist.init_process_group("nccl", device_id=torch.device("cuda", local))
        else:
            tdist.init_process_group(backend)
    dev = torch.device("cuda", local)
    torch.cuda.set_device(dev)
    ctx = Ctx(dev, rank, world, dist)

    if args.train:
        res = measure_train(ctx, args, args.model if args.model != "res15" else "res26-narrow", args.batch,
                            dump=args.dump_outputs)
        if rank == 0:
            res.update({"n_gpus": world, "steps": args.steps, "warmup": args.warmup, "higher_is_better": True,
                        "scaling": "weak", "vs_baseline": None,
                        "data": "synthetic N(0,1) [B,101,40] inputs + uniform labels resident in HBM"})
            print(json.dumps(res), flush=True)
        if dist:
            tdist.destroy_process_group()
        return

    from honk_amd import model as hm
    from oracle import ref_numpy as orc
    cfg = dict(hm.find_config(args.model))
    model = bench_model(args.model, dev)
    is_res = args.model.startswith("res")
    req = args.precision or "auto"   # what the reference's unchanged callers run
    if not is_res and req not in ("auto", "f32", "bf16x3"):
        raise SystemExit("cnn models: --precision auto, f32 or bf16x3")
    model.honk_precision = req
    B = args.batch or (131072 if is_res else 65536)
    g = torch.Generator(device=dev).manual_seed(1234 + rank)
    x = mfcc_like(B, dev, g)  # resident in HBM before timing
    log(f"world {world}: {args.model} {req} x {B} clips/GPU, {args.steps} steps")
    if args.e2e:  # raw 1 s PCM windows instead of MFCC maps; MFCC runs on the GPU inside the step
        from honk_amd.audio import AudioPreprocessor
        ap = AudioPreprocessor()
        pcm = (torch.rand(B, 16000, device=dev, generator=g) * 2 - 1) * 0.3

        def step_fn(p):
            return model(ap.compute_mfccs_batch(p))
        el, per, out, (kms, nlaunch, kflop) = ctx.timed(step_fn, pcm, args.steps, args.warmup)
        parity = None
        if args.full:
            idx = list(range(0, B, max(1, B // 32)))[:32]
            xs = ap.compute_mfccs_batch(pcm[idx])
            ref = orc.forward({k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}, cfg,
                              xs.cpu().numpy())
            got = out[idx].cpu().numpy()
            parity = {"top1_agreement_vs_oracle": float(np.mean(ref.argmax(1) == got.argmax(1))),
                      "max_abs_logit_err_vs_oracle_f64": float(np.abs(ref - got).max()), "sample_clips": len(idx)}
    else:
        with torch.no_grad():
            model(x[:8])   # resolve the precision request (the policy's one-off probe) before any timing
        el, per, out, (kms, nlaunch, kflop) = ctx.timed(model, x, args.steps, args.warmup)
        parity = _sample_parity(model, cfg, x, out, orc, B) if args.full else None
    prec = model.honk_last_precision   # the mode the request resolved to (the policy's choice)
    rerun = getattr(model, "honk_last_rerun", 0) if is_res else 0
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, {"logits": out}, rank, world)

    alts = {}
    extras = args.full and not args.no_alt and not args.e2e   # a plain run: the headline alone
    if extras:
        if is_res:
            for other in ("bf16x3", "f16x2", "f32", "bf16"):
                if other != prec:
                    log(f"res {other} mode")
                    alts[f"{other}_mode"] = measure_res(ctx, args, args.model, other, B, x=x, model=model)
    if extras and not args.no_configs:
        del x
        torch.cuda.empty_cache()
        log("C2 cnn-trad-pool2")
        alts["c2_cnn_trad_pool2"] = measure_c2(ctx, args)
        torch.cuda.empty_cache()
        log("C3 res8 bf16")
        c3 = measure_res(ctx, args, "res8", "bf16", 131072)
        c3["workload"] = "res8 eval forward in bf16 (config C3), 131,072 clips per GPU (1M over 8 GPUs)"
        alts["c3_res8_bf16"] = c3
        torch.cuda.empty_cache()
        log("C5 res26-narrow training")
        alts["c5_res26_narrow_train"] = measure_train(ctx, args)

    value = world * B * args.steps / el
    flop_clip = orc.flops_per_clip(cfg)
    if is_res:
        roof = res_roofline(prec, cfg, kms, nlaunch, kflop, B, args.model,
                            ctx.native.res_launch_plan(model._desc(101, 40, prec), B), args.steps)
    else:
        avg_ms = kms / max(nlaunch, 1)
        ach = (kflop / max(nlaunch, 1)) / (avg_ms * 1e-3) / 1e12 if nlaunch else None
        roof = {"bound": "mfma",
                "kernel": ("honk::cnn conv kernels in fp32 (conv1f_kernel + conv2f_kernel where the shapes fit, "
                           "else conv_gemm_kernel implicit GEMM; fp32 MFMA)"
                           if prec == "f32" else
                           "honk::cnn conv kernels in bf16x3 (3 bf16 MFMA products per MAC; peak = bf16 peak / 3)"),
                "achieved": round(ach, 2) if ach else None, "peak": round(MODE_PEAK[prec], 1), "unit": "TFLOP/s",
                "frac": round(ach / MODE_PEAK[prec], 4) if ach else None, "traffic": None,
                "launches": nlaunch, "avg_launch_ms": round(avg_ms, 4), "flop_per_launch": kflop / max(nlaunch, 1)}
    cpu = None
    if rank == 0 and args.full and not args.no_cpu_baseline:
        log("cpu baseline")
        cpu = cpu_baseline(cfg, args.cpu_seconds)
    if rank == 0:
        res = {
            "metric": METRIC,
            "value": round(value, 1),
            "unit": "clips/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(el / args.steps * 1e3, 3),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": prec,
            "precision_request": req,
            "precision_note": PREC_NOTES[prec],
            "data": "synthetic MFCC-like [B,101,40] fp32 input resident in HBM (c0 ~ N(-30, 20^2), c_k ~ "
                    "N(0, (8/(1+k))^2)); random-init weights (torch.manual_seed(0)), res BatchNorm statistics "
                    "calibrated on MFCC-like clips",
            "config": {"workload": ("PCM -> GPU MFCC -> " if args.e2e else "")
                                   + WORKLOADS.get(args.model, f"{args.model} eval forward"),
                       "per_gpu_batch": B, "global_batch": world * B,
                       "parallelism": f"batch-shard x{world} (no data-path collective)"},
            "per_rank_clips_s": [round(B * args.steps / t, 1) for t in per],
            "model_tflops": round(value * flop_clip / 1e12, 2),
            "roofline": roof,
        }
        if parity is not None:
            res["parity"] = parity
        if is_res:
            res["f16x2_admission"] = {"rerun_clips_last_step": rerun, "z_max": 8,
                                      "what": "every f16x2 batch is admitted per clip (tail_sum_kernel's flag, "
                                              "flag_compact_kernel, one host sync per call); flagged clips "
                                              "re-run in bf16x3 -- inside the timed steps"}
            if args.full and args.model == "res15" and not args.e2e:
                try:
                    res["f16x2_admission"]["fixtures"] = admission_report(dev)
                except Exception as e:  # a report, not the measurement
                    res["f16x2_admission"]["fixtures"] = {"error": repr(e)}
        res.update(alts)
        if cpu is not None:
            res["cpu_baseline"] = cpu
        res["modes"] = modes_summary(res, args.model)   # last: the compact view survives a cut tail
        print(json.dumps(res), flush=True)
    if dist:
        tdist.barrier()
        tdist.destroy_process_group()


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    args = parse(argv)
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        sys.exit(spawn_ranks(args.gpus, argv))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if args.gpus != world:
        log(f"note: --gpus {args.gpus} but WORLD_SIZE={world}; measuring {world} rank(s)")
    rank_main(args)


if __name__ == "__main__":
    main()
