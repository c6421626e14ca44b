#!/usr/bin/env python3
"""Headline benchmark: wall-clock SVM training time to tol=1e-3 on the MNIST
even/odd shape (60000 x 784, RBF, C=10, gamma=0.25) — BASELINE.json's metric.

  python bench.py --gpus N --steps K --warmup W
  (N > 1: either under python -m torch.distributed.run --nnodes=1
          --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py
          --gpus N ..., or plain `bench.py --gpus N`, which starts those N
          ranks itself before touching the GPU and relays rank 0's line; a
          rank count other than N is an error, never a silent downgrade)

One "step" = one complete training run from alpha = 0 to convergence: state
init, the resident Gram shard (MFMA GEMM) and the device-resident SMO loop —
the reference's timed region (svmTrainMain.cpp:206-314) plus the kernel-row
work it does inside that loop.  X upload / |x|^2 / cache allocation (the
reference's untimed setup, svmTrainMain.cpp:194-202) happen once, before.
W untimed warmup runs, then K timed runs bracketed by barrier + device sync;
the per-run time is the MAX over ranks.  Data: synthetic MNIST-shape (no
dataset or network on the box), identical on every rank (seeded).
Strong scaling: the problem is fixed.  Ranks split the rows (dp_policy
"shard"), or — the auto policy when the whole Gram fits one GPU — every rank
solves the whole problem (dp_policy "replicate": the SMO iteration is a latency
chain and sharding adds a cross-device hop to each of its ~10^5 iterations);
then one untimed sharded solve runs first and its time, iterations and b are
reported as "shard_check" (docs/DESIGN.md, Multi-GPU).

A plain run (--gpus 1 --steps K --warmup W) does what the headline figure
needs and no more: setup, W warmup solves, the K timed solves, the JSON line
(ms_per_step = milliseconds per timed solve).  --full adds everything else the
record can carry, untimed, after the timed solves: the training accuracy of
the timed model, the pair-at-a-time engine's solve of the same problem
("reference_check") and the structured mnist-parity problem ("secondary");
--reference-check off / --secondary off / --no-accuracy drop single parts of
it.  (N > 1: the policy measurement above picks the timed path, so it stays.)
--dump-outputs DIR writes what the last timed solve returned (alpha, b) as
DIR/<name>.npy; the inputs are seeded, so two builds given the same arguments
can be compared output for output.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

BASELINE_1GPU_S = 137.0   # README.md:23 (1x GTX 780)
BASELINE_MULTI_S = 46.0   # README.md:23 (10 GPUs, OpenMPI over Ethernet)
METRIC = "wall-clock training time (s) to tol=1e-3, MNIST even-odd RBF, at 1/2/4/8 MI355X"

# BASELINE.json configs (parameters from README.md:23 and Makefile:74-86)
PRESETS = {
    "mnist": dict(data="mnist", samples=60000, features=784, C=10.0, gamma=0.25, eps=1e-3, max_iter=150000),
    "mnist-makefile": dict(data="mnist", samples=60000, features=784, C=10.0, gamma=0.125, eps=0.01,
                           max_iter=100000),
    "mnist-parity": dict(data="mnist-parity", samples=60000, features=784, C=10.0, gamma=0.25, eps=1e-3,
                         max_iter=150000),
    "adult": dict(data="adult", samples=32561, features=123, C=100.0, gamma=0.5, eps=1e-3, max_iter=150000),
    "covtype": dict(data="covtype", samples=581012, features=54, C=2048.0, gamma=0.03125, eps=1e-3,
                    max_iter=3000000),
    # Makefile:77 (run_cover): the first 500,000 covtype rows
    "covtype-ref": dict(data="covtype", samples=500000, features=54, C=2048.0, gamma=0.03125, eps=1e-3,
                        max_iter=3000000),
    "synthetic-2m": dict(data="uniform", samples=2000000, features=1024, C=1.0, gamma=1.0 / 1024, eps=1e-3,
                         max_iter=3000000),
}


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also run the untimed extras: training accuracy, the "
                         "reference_check solve and the secondary problem (a plain run skips them)")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="write the last timed step's outputs (alpha, b) as DIR/<name>.npy")
    ap.add_argument("--config", default="mnist", choices=sorted(PRESETS),
                    help="preset (BASELINE.json configs; explicit flags override)")
    ap.add_argument("--data", default=None, help="synthetic generator (mnist = BASELINE headline shape)")
    ap.add_argument("--samples", type=int, default=None)
    ap.add_argument("--features", type=int, default=None)
    ap.add_argument("--C", type=float, default=None)
    ap.add_argument("--gamma", type=float, default=None)
    ap.add_argument("--eps", type=float, default=None)
    ap.add_argument("--max-iter", type=int, default=None)
    ap.add_argument("--host-cache-lines", type=int, default=0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--cache-lines", type=int, default=0)
    ap.add_argument("--clip", default="independent", choices=["independent", "box"],
                    help="alpha clipping: the reference's independent clip (default) or the joint box")
    ap.add_argument("--cache-mb", type=float, default=0,
                    help="cap the kernel-row cache / resident Gram budget per rank (MiB; ranks sharing a device)")
    ap.add_argument("--x-mode", default="auto")
    ap.add_argument("--graph-block", type=int, default=64)
    ap.add_argument("--comm", default="auto", help="auto | rccl | gloo")
    ap.add_argument("--exchange", default="auto", choices=["auto", "allreduce", "peer"],
                    help="per-iteration key exchange of the dense mode (auto: in-kernel xGMI peer exchange "
                         "when its self test passes, else the communicator all-reduce)")
    ap.add_argument("--device", default="auto", help="auto | cuda | cpu")
    ap.add_argument("--persist", default="auto", choices=["auto", "off", "on"],
                    help="iteration engine: persistent kernel (auto/on; dense and cache mode) or one launch per iteration (off)")
    ap.add_argument("--persist-block", type=int, default=2048)
    ap.add_argument("--dp", default="auto", choices=["auto", "shard", "replicate", "measure"],
                    help="data parallelism at N > 1: shard the rows, or every rank solves the whole problem "
                         "(auto: replicate when the whole Gram fits one GPU, docs/DESIGN.md — then both "
                         "policies are timed once on this node and the timed runs use the faster; measure: "
                         "that measured choice whatever the shape-based policy says)")
    ap.add_argument("--secondary", default="auto", choices=["auto", "off"],
                    help="--full, headline config at N=1: also record the structured mnist-parity problem (untimed for the headline)")
    ap.add_argument("--shard-check", default="auto", choices=["auto", "off"],
                    help="N > 1 with a replicated timed solve: one untimed sharded solve first (cross-device "
                         "exchange evidence: its time, iterations and b go into the JSON line)")
    ap.add_argument("--solver", default="auto", choices=["auto", "smo", "ws"],
                    help="auto (default, the library's and svmTrain's default): working-set rounds from 50k rows "
                         "(the reference's pair rule on q-row sub-problems in LDS, the reference's stop test on "
                         "the exact gradient), else the pair-at-a-time engines; ws / smo force one of them")
    ap.add_argument("--reference-check", default="auto", choices=["auto", "off"],
                    help="--full: when the timed solve ran ws-dense, one untimed solve by the pair-at-a-time engine (the reference's "
                         "trajectory) after the timed runs; its time, iterations, b, support vectors and the "
                         "decision agreement with the timed model go into the JSON line")
    ap.add_argument("--ws-size", type=int, default=192)
    ap.add_argument("--ws-new", type=int, default=0)
    ap.add_argument("--ws-rel", type=float, default=0.3)
    ap.add_argument("--ws-inner", type=int, default=0, help="pair steps per block and round at most (0: 4 ws_size)")
    ap.add_argument("--ws-block", type=int, default=8)
    ap.add_argument("--ws-t-halve", type=float, default=None, help="multi-block: damped rounds below this t halve P")
    ap.add_argument("--shrink", default="auto", choices=["auto", "on", "off"],
                    help="one GPU: LIBSVM-style shrinking as problem reduction (phases on the active rows); "
                         "auto (the library's default): on when the whole Gram is not resident (C.shrink_auto)")
    ap.add_argument("--ws-no-clip-fallback", action="store_true",
                    help="multi-block, independent clipping: keep the blocks after a clip event")
    ap.add_argument("--ws-wss", type=int, default=None, choices=[0, 1, 2],
                    help="sub-problem pair choice: 1 first order (the reference's rule), 2 second order (WSS2), "
                         "0 auto (second order when the kernel couples rows); default: the library's (auto)")
    ap.add_argument("--ws-blocks", type=int, default=0,
                    help="up to P sub-problems solved per round on separate workgroups, combined by a line search "
                         "(1..32; 0 = the library default: 32 blocks of 96 rows from 50k rows, halved after every "
                         "damped round)")
    ap.add_argument("--eta", default="x", choices=["x", "gram"],
                    help="pair-at-a-time engines: K(hi, lo) of eta from the two X rows (default) or the resident Gram")
    ap.add_argument("--gram", default="auto", choices=["auto", "f32", "split"],
                    help="Gram / kernel-row GEMMs: f32-input MFMA or fp16 MFMA over hi/lo split operands (fp32 "
                         "accuracy); auto = split for the working-set engines")
    ap.add_argument("--gram-adapt", default="auto", choices=["auto", "on", "off"],
                    help="resident ws-dense Gram: one-product tiles where every value is provably within 2^-22 of "
                         "the three-product split value, the rest recomputed (docs/DESIGN.md §13); auto = on when "
                         "a row sample passes the bound")
    ap.add_argument("--rows-per-group", type=int, default=0, help="engine geometry override (multiple of 256)")
    ap.add_argument("--cache-groups", type=int, default=256)
    ap.add_argument("--force-cache", action="store_true")
    ap.add_argument("--engines", default="production", choices=["production", "all"],
                    help="all: also the quarantined pair-at-a-time cache / partitioned-X engines (A/B probes; "
                         "--host-cache-lines needs it)")
    ap.add_argument("--xch-poll-batch", type=int, default=0)
    ap.add_argument("--xch-mem", default="auto", choices=["auto", "uncached", "coarse"])
    ap.add_argument("--xch-timeout", type=float, default=None,
                    help="give-up bound of one in-kernel exchange poll (default 30 s at N > 1, else 120 s)")
    ap.add_argument("--no-accuracy", action="store_true", help="--full without the training accuracy")
    ap.add_argument("--log-every", type=int, default=0,
                    help="rank 0 prints b_hi / b_lo / gap every N pair steps (long big-config runs)")
    ap.add_argument("--verbose", action="store_true", help="solver diagnostics on stderr (engine, shrink phases)")
    ap.add_argument("--json-out", default=None)
    a = ap.parse_args(argv)
    for k, v in PRESETS[a.config].items():
        if getattr(a, k) is None:
            setattr(a, k, v)
    return a


def _free_port() -> int:
    import socket

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _visible_devices() -> int:
    """Device count WITHOUT initialising the GPU (torch.cuda.device_count()
    does not on this image; is_available() would)."""
    try:
        import torch

        return int(torch.cuda.device_count())
    except Exception:  # noqa: BLE001
        return 0


def spawn_ranks(a, argv) -> int:
    """``--gpus N`` (N > 1) outside a torch.distributed launch: start the N
    ranks ourselves — one process per GPU over torch.distributed.run, the
    replacement of the reference's ``mpirun -np P`` (Makefile:74) — and relay
    rank 0's JSON line.  Runs BEFORE anything touches the GPU (this process
    never initialises HIP, and it never exec()s: the ranks are children).
    Fails non-zero when a rank fails, no JSON line arrives, or the line does
    not report N ranks — never a silent one-rank downgrade."""
    import subprocess

    n = a.gpus
    if a.device != "cpu":
        have = _visible_devices()
        shared = os.environ.get("DPSVM_FORCE_DEVICE")
        if (a.device == "cuda" or have > 0) and have < n and not shared:
            print(f"[bench] --gpus {n} but only {have} visible device(s); set DPSVM_FORCE_DEVICE=<id> "
                  f"to rehearse {n} ranks sharing one device", file=sys.stderr)
            return 2
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    if os.environ.get("DPSVM_FORCE_DEVICE"):
        # rehearsal: N ranks share one device.  With HIP's default of 4 hardware
        # queues per process, 8 processes oversubscribe the device's queues and the
        # scheduler time-slices them: a round's spinning consumers then wait out
        # whole quanta for a descheduled peer's pushes (8-rank headline 2.30 s
        # vs 0.065 s with 2 queues each, profiles/r5_rehearsal_queues_1gpu.txt).
        # Overridden even when the environment sets it (the GPU boxes export 4)
        env["GPU_MAX_HW_QUEUES"] = os.environ.get("DPSVM_REHEARSAL_HW_QUEUES", "2")
    env["DPSVM_BENCH_SPAWNED"] = str(n)
    cmd = [sys.executable, "-u", "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
           os.path.abspath(__file__), *argv]
    print(f"[bench] spawning {n} ranks: {' '.join(cmd[2:])}", file=sys.stderr, flush=True)
    proc = subprocess.Popen(cmd, stdout=subprocess.PIPE, env=env, text=True, bufsize=1)
    result = None
    for line in proc.stdout:
        s = line.strip()
        if s.startswith("{"):
            try:
                result = json.loads(s)
            except ValueError:
                print(line, end="", file=sys.stderr)
                continue
        else:
            print(line, end="", file=sys.stderr, flush=True)  # rank chatter: keep stdout one JSON line
    rc = proc.wait()
    if rc != 0:
        print(f"[bench] a rank failed (torch.distributed.run exit {rc})", file=sys.stderr)
        return rc if rc > 0 else 1
    if result is None:
        print("[bench] no JSON line from rank 0", file=sys.stderr)
        return 1
    if int(result.get("n_gpus", 0)) != n:
        print(f"[bench] rank 0 reported n_gpus={result.get('n_gpus')} for --gpus {n}", file=sys.stderr)
        return 1
    result["launcher"] = "bench.py spawned torch.distributed.run"
    line = json.dumps(result)
    print(line, flush=True)
    if a.json_out:
        with open(a.json_out, "w") as f:
            f.write(line + "\n")
    return 0


DUMP_LIMIT_BYTES = 64 << 20  # --dump-outputs: all files together


def dump_outputs(dirname, arrays) -> None:
    """Write each array as <dirname>/<name>.npy in float32 (float64 stays
    float64).  Past DUMP_LIMIT_BYTES in all, every array keeps a fixed, seeded
    sample of its flattened elements (the same indices for the same shapes)."""
    import numpy as np

    os.makedirs(dirname, exist_ok=True)
    arrs = {}
    for name, v in arrays.items():
        v = np.asarray(v)
        arrs[name] = np.ascontiguousarray(v if v.dtype == np.float64 else v.astype(np.float32))
    total = sum(v.nbytes for v in arrs.values())
    budget = DUMP_LIMIT_BYTES - 4096 * len(arrs)  # room for the .npy headers
    for name, v in arrs.items():
        if total > budget:
            keep = max(1, int(v.size * (budget / total)))
            idx = np.sort(np.random.default_rng(0).choice(v.size, size=keep, replace=False))
            v = v.reshape(-1)[idx]
        np.save(os.path.join(dirname, name + ".npy"), v)


def main(argv=None) -> int:
    raw_argv = list(sys.argv[1:] if argv is None else argv)
    a = parse(raw_argv)
    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        return spawn_ranks(a, raw_argv)
    if a.gpus < 1:
        raise SystemExit("--gpus must be >= 1")
    if a.steps < 1:
        raise SystemExit("--steps must be >= 1")
    import numpy as np
    import torch
    import torch.distributed as dist

    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from dpsvm_amd import SVCConfig
    from dpsvm_amd._native import load
    from dpsvm_amd.parallel import init_distributed, make_comm, shutdown
    from dpsvm_amd.utils.datasets import synthetic

    multi = int(os.environ.get("WORLD_SIZE", "1")) > 1
    # (N > 1: the solver checks a cross-rank alpha digest after every run, so a
    # diverged run fails loudly instead of reporting a time)
    C = load()
    if a.engines == "all":
        from dpsvm_amd._native import load_quarantine

        load_quarantine()  # the quarantined pair-at-a-time cache engines (plugin)
    ctx = init_distributed(device=a.device)
    on_gpu = ctx.device.startswith("cuda")

    def barrier():
        if ctx.world > 1:
            dist.barrier()

    def sync():
        if on_gpu:
            torch.cuda.synchronize()

    if ctx.world != a.gpus:
        # never benchmark a different rank count than asked for
        raise SystemExit(f"[bench] --gpus {a.gpus} but WORLD_SIZE={ctx.world}")
    n_ranks = ctx.world

    X, y = synthetic(a.data, n=a.samples, d=a.features, seed=a.seed)
    cfg = SVCConfig(C=a.C, gamma=a.gamma, eps=a.eps, max_iter=a.max_iter, cache_lines=a.cache_lines, cache_mb=a.cache_mb,
                    clip=a.clip,
                    x_mode=a.x_mode, graph_block=a.graph_block, host_cache_lines=a.host_cache_lines,
                    exchange=a.exchange, persist=a.persist, persist_block=a.persist_block,
                    dp="replicate" if a.dp == "measure" else a.dp,
                    rows_per_group=a.rows_per_group, cache_groups=a.cache_groups, force_cache=a.force_cache, engines=a.engines,
                    xch_poll_batch=a.xch_poll_batch, xch_mem=a.xch_mem, solver=a.solver, ws_size=a.ws_size,
                    ws_new=a.ws_new, ws_rel=a.ws_rel, ws_block=a.ws_block, ws_blocks=a.ws_blocks, ws_inner=a.ws_inner, eta=a.eta,
                    gram=a.gram, gram_adapt=a.gram_adapt,
                    **({} if a.ws_wss is None else {"ws_wss": a.ws_wss}),
                    **({} if a.ws_t_halve is None else {"ws_t_halve": a.ws_t_halve}),
                    **({"ws_clip_fallback": False} if a.ws_no_clip_fallback else {}),
                    xch_timeout_s=a.xch_timeout if a.xch_timeout is not None else (30.0 if multi else 120.0))
    params = cfg.to_native(X.shape[1])
    if ctx.rank == 0:
        params.log_every = a.log_every
        params.verbose = a.verbose
    # auto: RCCL, or gloo on EVERY rank when the RCCL bootstrap fails on any
    # rank (agreed over the host group, dpsvm_amd.parallel.make_comm); the
    # per-iteration exchange is in-kernel either way
    comm = make_comm(ctx, a.comm)
    if a.comm == "rccl" and n_ranks == 1:
        params.force_collectives = True  # one-rank RCCL: exercise the collective + graph path

    def progress(it, bh, bl, el, hits, misses):
        print(f"[bench] iter {it} b_hi {bh:.6g} b_lo {bl:.6g} gap {bl - bh:.3g} {el:.1f} s "
              f"hits {hits} misses {misses}", file=sys.stderr, flush=True)

    sh_comm = comm if n_ranks > 1 else None
    use_shrink = on_gpu and (a.shrink == "on" or (
        a.shrink == "auto" and C.shrink_auto(params, X.shape[0], X.shape[1], ctx.local_rank, sh_comm)))
    if use_shrink:
        # shrinking phases: the whole-problem solver is set up here, untimed, as the
        # plain solver is (X upload, cache sizing); every shrunk phase sets its
        # (multi-rank) solver up inside the timed run
        solver = None
        shr = C.ShrinkingSolver(params, sh_comm, ctx.local_rank)
        info = shr.setup(X, y)
        if n_ranks > 1:
            info["dp_policy"] = f"per phase ({a.dp}; whole problem: {info['dp_policy']})"
        run = lambda: shr.solve(None, progress if (a.log_every and ctx.rank == 0) else None)  # noqa: E731
    elif on_gpu:
        solver = C.GpuSolver(params, comm, ctx.local_rank)
        info = solver.setup(X, X.shape[0], y)

        if a.log_every and ctx.rank == 0:
            run = lambda: solver.solve(None, progress)  # noqa: E731
        else:
            run = lambda: solver.solve()  # noqa: E731
        if n_ranks > 1 and info.get("exchange") == "peer" and a.exchange == "auto":
            # the in-kernel peer exchange is self-tested at setup; if a warmup run still
            # fails on it (every rank fails the same way), fall back to the collective path
            try:
                run()
            except C.NativeError as e:
                if ctx.rank == 0:
                    print(f"[bench] peer exchange run failed ({e}); falling back to the all-reduce",
                          file=sys.stderr)
                del solver
                cfg.exchange, cfg.persist = "allreduce", "off"
                params = cfg.to_native(X.shape[1])
                solver = C.GpuSolver(params, comm, ctx.local_rank)
                info = solver.setup(X, X.shape[0], y)
                run = lambda: solver.solve()  # noqa: E731
    else:
        info = {"device_name": "cpu", "x_replicated": True, "cache_lines": 0}
        run = lambda: C.solve_cpu(X, y, params, comm if n_ranks > 1 else None)  # noqa: E731

    def timed_once(fn):
        """one solve bracketed by barrier + device sync; the max over ranks"""
        sync()
        barrier()
        t_s = time.perf_counter()
        r = fn()
        sync()
        barrier()
        tt = torch.tensor([time.perf_counter() - t_s], dtype=torch.float64)
        if n_ranks > 1:
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)  # host (gloo) group: every rank sees the same value
        return float(tt[0]), r

    shard_check = None
    dp_choice = None
    s_solver = s_comm = None
    s_info = None
    if on_gpu and n_ranks > 1 and info.get("dp_policy") == "replicate" and a.shard_check == "auto":
        # the replicated policy (every rank solves it all) was chosen from the
        # problem's shape; prove the sharded, cross-device path on this node too
        # (one untimed solve), and with --dp auto MEASURE both policies: the
        # timed runs use the faster one on this node (the choice is made from
        # max-over-ranks times, identical on every rank)
        sp = cfg.to_native(X.shape[1])
        sp.dp_policy = 1
        sp.watchdog_s = 120.0  # a stuck collective aborts ITS communicator and fails this check only
        try:
            s_comm = make_comm(ctx, comm.name if comm.name in ("rccl", "gloo") else "auto")
            s_solver = C.GpuSolver(sp, s_comm, ctx.local_rank)
            s_info = s_solver.setup(X, X.shape[0], y)
            t_first, (s_alpha, s_res) = timed_once(s_solver.solve)
            shard_check = {"s": round(t_first, 6), "iterations": int(s_res["iters"]),
                           "b": s_res["b"], "smo_loop_s": round(float(s_res["t_solve"]), 6),
                           "gram_gemm_s": round(float(s_res.get("t_gram", 0.0)), 6),
                           "engine": s_info.get("iteration"), "exchange": s_info.get("exchange"),
                           "ws_exchange": s_info.get("ws_exchange"), "engine_note": s_info.get("engine_note", ""),
                           "exchange_mem": s_info.get("exchange_mem"),
                           "geometry": f"{s_info.get('rows_per_group')}x{s_info.get('groups')}",
                           "us_per_iter": round(1e6 * float(s_res["t_solve"]) / max(1, int(s_res["iters"])), 3),
                           "verified": True}
            del s_alpha
            if a.dp in ("auto", "measure"):
                t_shard, _ = timed_once(s_solver.solve)  # warm (graphs instantiated)
                for _ in range(max(1, a.warmup)):
                    run()
                t_repl, _ = timed_once(run)
                use_shard = t_shard < 0.97 * t_repl
                dp_choice = {"replicate_s": round(t_repl, 6), "shard_s": round(t_shard, 6),
                             "chosen": "shard" if use_shard else "replicate"}
                if use_shard:
                    solver, info = s_solver, s_info
                    run = lambda: solver.solve()  # noqa: E731
                    comm = s_comm
        except Exception as e:  # noqa: BLE001  (the digest inside solve() fails on every rank alike)
            shard_check = {"error": str(e)[:300]}
            if ctx.rank == 0:
                print(f"[bench] sharded check failed: {e}", file=sys.stderr)
        if dp_choice is None or dp_choice["chosen"] != "shard":
            s_solver = None
            s_comm = None


    for _ in range(a.warmup):
        run()
    barrier()
    sync()
    t0 = time.perf_counter()
    results = [run() for _ in range(a.steps)]
    sync()
    barrier()
    elapsed = time.perf_counter() - t0
    per_run = elapsed / a.steps
    solve_s = [r[1]["t_solve"] for r in results]
    t = torch.tensor([per_run, max(solve_s), min(solve_s)], dtype=torch.float64)
    if n_ranks > 1:
        t[2] = -t[2]
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        t[2] = -t[2]
    per_run, solve_max, solve_min = t.tolist()
    alpha, res = results[-1]
    if a.dump_outputs and ctx.rank == 0:
        dump_outputs(a.dump_outputs, {"alpha": alpha, "b": [res["b"]]})
    acc = None
    if a.full and not a.no_accuracy and on_gpu and solver is not None:
        acc = float(solver.train_accuracy(alpha, res["b"]))
    nsv = int((alpha > 0).sum())
    ref_check = None
    if (a.full and on_gpu and a.solver != "smo" and a.reference_check == "auto" and info.get("iteration") == "ws-dense"
            and (n_ranks == 1 or info.get("dp_policy") == "replicate")):
        rows = np.arange(0, X.shape[0], max(1, X.shape[0] // 4096))
        d_ws = np.asarray(solver.decision(alpha, res["b"], X[rows]))
        del solver  # its resident Gram: the cross-check builds its own
        # the same problem by the pair-at-a-time engine (the reference's exact
        # trajectory, svmTrainMain.cpp:235-310), untimed: the two models must agree
        rp = cfg.to_native(X.shape[1])
        rp.solver = 1
        r_solver = C.GpuSolver(rp, comm, ctx.local_rank)
        r_info = r_solver.setup(X, X.shape[0], y)
        sync()
        t_r = time.perf_counter()
        r_alpha, r_res = r_solver.solve()
        sync()
        t_r = time.perf_counter() - t_r
        d_ref = np.asarray(r_solver.decision(r_alpha, r_res["b"], X[rows]))
        ref_check = {"engine": r_info.get("iteration"), "s": round(t_r, 6), "iterations": int(r_res["iters"]),
                     "converged": bool(r_res["converged"]), "b": r_res["b"], "abs_b_diff": abs(r_res["b"] - res["b"]),
                     "n_sv": int((r_alpha > 0).sum()), "decision_sign_agreement": float(np.mean(
                         np.sign(d_ws) == np.sign(d_ref))), "rows_compared": int(len(rows))}
        del r_solver

    secondary = None
    headline_cfg = a.config == "mnist" and a.data == "mnist" and a.samples == 60000 and a.features == 784
    if a.full and on_gpu and n_ranks == 1 and headline_cfg and a.secondary == "auto" and ctx.rank == 0:
        # the headline data is degenerate (K ~ I: every row a support vector); the
        # structured MNIST-shape problem of the same size and parameters
        # (mnist-parity: digit-like prototypes, label = parity) rides along in the
        # same record, untimed for the headline: its own median of 3 solves
        Xp, yp = synthetic("mnist-parity", n=a.samples, d=a.features, seed=a.seed)
        sp_solver = C.GpuSolver(cfg.to_native(Xp.shape[1]), None, ctx.local_rank)
        sp_solver.setup(Xp, Xp.shape[0], yp)
        sp_solver.solve()  # warmup (graphs instantiated)
        ts, sres = [], None
        for _ in range(3):
            sync()
            t_s = time.perf_counter()
            s_alpha, sres = sp_solver.solve()
            sync()
            ts.append(time.perf_counter() - t_s)
        secondary = {"config": "mnist-parity", "data": "synthetic mnist-parity-shape 60000x784 (digit-like prototypes, "
                     "label = parity)", "value": round(float(np.median(ts)), 6), "unit": "s",
                     "rounds": int(sres.get("outer", 0)), "iterations": int(sres["iters"]),
                     "converged": bool(sres["converged"]), "n_sv": int((s_alpha > 0).sum()), "b": sres["b"],
                     "train_accuracy": float(sp_solver.train_accuracy(s_alpha, sres["b"]))}
        del sp_solver

    def rank_diag(inf):
        """this rank's setup as the timed solver ran it (N > 1: gathered to rank 0)"""
        if not isinstance(inf, dict):
            return None
        return {"rank": ctx.rank, "device": inf.get("device"), "comm": inf.get("comm_kind"),
                "n_local": inf.get("n_local"), "dp_policy": inf.get("dp_policy"), "engine": inf.get("iteration"),
                "exchange": inf.get("exchange"), "ws_exchange": inf.get("ws_exchange"),
                "exchange_mem": inf.get("exchange_mem"), "xch_selftest": inf.get("xch_selftest", ""),
                "union": f"{inf.get('ws_blocks', 0)}x{inf.get('ws_q_max', 0)}",
                "bytes_device": inf.get("bytes_device"), "engine_note": inf.get("engine_note", "")}

    rank_setup = None
    if n_ranks > 1:
        # per-rank setup diagnostics (exchange self test, uncached receive buffer,
        # union, communicator): a first multi-GPU failure is readable from the line
        rank_setup = [None] * n_ranks
        from dpsvm_amd.parallel.dist import _host_group

        dist.all_gather_object(rank_setup, {"timed": rank_diag(info), "shard_check": rank_diag(s_info)},
                               group=_host_group())
    policy = info.get("dp_policy", "shard")
    if n_ranks > 1 and dp_choice is None:
        # always both data-parallel policies' times at N > 1 where measured: the
        # sharded time next to a replicated one (a replicated solve is not a
        # scaling point), the timed run's own time for the policy it used
        dp_choice = {"replicate_s": round(per_run, 6) if policy == "replicate" else None,
                     "shard_s": (round(per_run, 6) if policy != "replicate" else
                                 (shard_check or {}).get("s")),
                     "chosen": "replicate" if policy == "replicate" else "shard"}
    if ctx.rank == 0:
        # the reference publishes numbers for the MNIST config only (README.md:23)
        headline = a.config == "mnist" and a.data == "mnist" and a.samples == 60000 and a.features == 784
        base = (BASELINE_1GPU_S if n_ranks == 1 else BASELINE_MULTI_S) if headline else None
        metric = METRIC if headline else (
            f"wall-clock training time (s) to tol={a.eps:g}, {a.data}-shape {a.samples}x{a.features} RBF")
        out = {
            "metric": metric,
            "value": round(per_run, 6),
            "unit": "s",
            "n_gpus": n_ranks,
            "steps": a.steps,
            "warmup": a.warmup,
            "full": bool(a.full),
            "ms_per_step": round(per_run * 1000.0, 3),
            "higher_is_better": False,
            "scaling": "strong",
            "vs_baseline": round(per_run / base, 6) if base else None,
            "speedup_vs_baseline": round(base / per_run, 2) if base else None,
            "baseline_s": base,
            "dtype": "fp32",
            "data": f"synthetic {a.data}-shape {a.samples}x{a.features} (seed {a.seed}; "
                    + ("pixel-like [0,1] features, random +/-1 labels)" if a.data == "mnist" else "generated)"),
            "config": {
                "model": f"RBF C-SVM, modified SMO (C={a.C:g}, gamma={a.gamma:g}, tol={a.eps:g})",
                "global_batch": a.samples,
                "seq_len": a.features,
                # dpN-shard: the rows split over N ranks (each rank a shard of f, Gram
                # columns / cache lines); replicateN: every rank solves the whole
                # problem (no communication; NOT a strong-scaling point)
                "parallelism": ("dp1" if n_ranks == 1 else
                                f"replicate{n_ranks}" if policy == "replicate" else f"dp{n_ranks}-shard"),
            },
            "iterations": int(res["iters"]),
            "rounds": int(res.get("outer", 0)),
            "ws_blocks": {"start": int(res.get("ws_blocks", 1)), "end": int(res.get("ws_blocks_end", 1)),
                          "one_block_from_round": int(res.get("ws_p1_round", 0)),
                          "damped_rounds": int(res.get("ws_damped", 0))},
            "converged": bool(res["converged"]),
            **({"note": "stopped at the iteration cap: an unconverged working-set model is not the reference's "
                        "pair-at-a-time iterate at the same cap (raise --max-iter to converge)"}
               if int(res["status"]) == 2 and int(res.get("outer", 0)) > 0 else {}),
            "n_sv": nsv,
            "b": res["b"],
            "b_hi": res.get("b_hi"),
            "b_lo": res.get("b_lo"),
            "final_gap": (res["b_lo"] - res["b_hi"]) if "b_lo" in res else None,  # stop: gap <= 2 eps
            "train_accuracy": acc,
            "gram_gemm_s": round(float(res.get("t_gram", 0.0)), 6),
            "smo_loop_s_min": round(solve_min, 6),
            "smo_loop_s_max": round(solve_max, 6),
            "iters_per_s": round(res["iters"] / max(solve_max, 1e-9), 1),
            "cache": {k: int(res.get(k, 0)) for k in ("cache_hits", "cache_misses", "x_passes", "rows_computed",
                                                       "spec_rows", "host_hits")},
            "device": info.get("device_name", ""),
            "x_replicated": bool(info.get("x_replicated", True)),
            "iteration": info.get("iteration", "cpu"),
            "gram": info.get("gram", "f32"),
            # adaptive Gram: one-product tiles and the hot ones recomputed with three products (-1: not adaptive)
            "gram_tiles": int(res.get("gram_tiles", -1)),
            "gram_hot_tiles": int(res.get("gram_hot_tiles", -1)),
            "cache_lines": int(info.get("cache_lines", 0)),
            "comm": getattr(comm, "name", "local"),
            "exchange": info.get("exchange", "none"),
            # working-set rounds: peer (in-kernel pushes) | collectives | loopback | none
            "ws_exchange": info.get("ws_exchange", "none"),
            "exchange_mem": info.get("exchange_mem", "none"),
            "dp_policy": info.get("dp_policy", "shard"),
            "geometry": f"{info.get('rows_per_group', 0)}x{info.get('groups', 0)}",
            "poll_batch": info.get("poll_batch", 0),
            "census": info.get("census", "n/a"),
            "engine_note": info.get("engine_note", ""),
            "shrink": {"mode": a.shrink, "on": bool(use_shrink), "phases": int(res.get("shrink_phases", 0)),
                       "whole_problem_engine": info.get("phase0_engine"),
                       "phase_log": res.get("phase_log", "")},
            "shard_check": shard_check,
            "dp_autotune": dp_choice,
            "rank_setup": rank_setup,
            "reference_check": ref_check,
            "secondary": secondary,
            "ws_rounds": info.get("ws_rounds", "none"),
            "ws_rows": info.get("ws_rows", "none"),
            "params": json.loads(params.to_json()),
            "preset": a.config,
        }
        line = json.dumps(out)
        print(line, flush=True)
        if a.json_out:
            with open(a.json_out, "w") as f:
                f.write(line + "\n")
    del comm
    shutdown(ctx)
    return 0


if __name__ == "__main__":
    sys.exit(main())
