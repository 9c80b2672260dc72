#!/usr/bin/env python3
"""Flagship benchmark: perf_analyzer-style serving throughput.

Measures the BASELINE.json north-star config: ResNet50 bs=8, bf16,
HIP-IPC shared-memory I/O, gRPC async clients, one MI355X-backed server
replica per GPU (one rank per GPU under torch.distributed.run).

Each rank: spawns a server process on its GPU, creates per-slot HIP-shm
input/output regions, registers them over gRPC, and drives closed-loop
async inference. A step = `reqs_per_step` requests at concurrency
`concurrency`; every step re-runs the CDNA4 pack kernel (fp32 -> bf16
into the slot-0 input region) and, when world_size > 1, RCCL-broadcasts
rank 0's staged input to every rank's region over xGMI before issuing
requests (BASELINE.md config 3/5 shape).

Rank 0 prints one JSON line (whole-job aggregate; weak scaling).

A plain run sets up, warms up, times `--steps` steps and prints that
line; nothing else is measured, so `--full` (reserved for extended
measurements) currently adds nothing. The synthetic input and the
server's model weights are seeded by `--seed`; `--dump-outputs DIR`
saves the output regions as the last timed step left them, for
comparing two builds output for output.
"""

import argparse
import atexit
import json
import os
import shutil
import subprocess
import sys
import tempfile
import threading
import time

import numpy as np

os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

BATCH = 8
IN_SHAPE = (BATCH, 3, 224, 224)
OUT_SHAPE = (BATCH, 1000)


def start_server(device_index, port, extra_args=(), seed=0):
    env = dict(os.environ)
    # one MIOpen find-db/cache per rank: 8 server processes sharing one
    # sqlite user-db serialize on its lock during warmup and can blow
    # the ready window (ROUND2_NOTES item 1)
    miopen_dir = f"/tmp/miopen_rank{device_index}"
    try:
        os.makedirs(miopen_dir, exist_ok=True)
    except OSError:
        pass
    if not os.access(miopen_dir, os.W_OK):
        # left behind by another user: take a directory of our own
        miopen_dir = os.path.join(
            tempfile.gettempdir(),
            f"miopen_rank{device_index}_uid{os.getuid()}")
        os.makedirs(miopen_dir, exist_ok=True)
    env.setdefault("MIOPEN_USER_DB_PATH", miopen_dir)
    env.setdefault("MIOPEN_CUSTOM_CACHE_DIR", miopen_dir)
    repo = os.path.dirname(os.path.abspath(__file__))
    # the checkout may be read-only: the server log goes to a temporary
    # directory that is removed when the benchmark exits
    log_dir = tempfile.mkdtemp(prefix="client_amd_bench_")
    atexit.register(shutil.rmtree, log_dir, ignore_errors=True)
    log_path = os.path.join(log_dir, f"server_rank{device_index}.log")
    log_f = open(log_path, "w")
    # the server random-initialises the model on the host; seeding torch
    # before it is built makes the weights, and so the outputs, the same
    # from run to run
    launcher = ("import sys, torch; torch.manual_seed(int(sys.argv.pop(1))); "
                "from client_amd.server.__main__ import main; "
                "main(sys.argv[1:])")
    proc = subprocess.Popen(
        [sys.executable, "-c", launcher, str(seed),
         "--grpc-port", str(port),
         "--models", "resnet50", "--device", f"cuda:{device_index}",
         "--dtype", "bf16", "--grpc-workers", "8", *extra_args],
        stdout=log_f, stderr=subprocess.STDOUT, text=True, env=env, cwd=repo,
    )
    deadline = time.time() + 300
    port_actual = None
    while time.time() < deadline:
        if proc.poll() is not None:
            raise RuntimeError(
                f"server exited early; log: {open(log_path).read()[-2000:]}"
            )
        try:
            with open(log_path) as f:
                for line in f:
                    if line.startswith("GRPC_READY"):
                        port_actual = int(line.split()[1])
                        break
        except FileNotFoundError:
            pass
        if port_actual is not None:
            break
        time.sleep(0.1)
    if port_actual is None:
        proc.terminate()
        raise RuntimeError("server did not become ready")
    return proc, port_actual


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--concurrency", type=int, default=8)
    ap.add_argument("--reqs-per-step", type=int, default=48)
    ap.add_argument("--no-dynamic-batching", action="store_true")
    ap.add_argument("--preferred-batch-size", type=int, default=32)
    ap.add_argument("--stagger-s", type=float, default=1.5,
                    help="per-rank server-spawn stagger (world>1)")
    ap.add_argument("--fanout", choices=("rccl", "p2p"),
                    default=os.environ.get("CLIENT_AMD_FANOUT", "rccl"),
                    help="8-way input replication: RCCL broadcast (tree "
                         "over xGMI) or 7-link hipMemcpyPeerAsync direct "
                         "scatter")
    ap.add_argument("--seed", type=int, default=0,
                    help="seeds the synthetic input and the server's model "
                         "weights, so runs with the same arguments compute "
                         "on identical data")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last step's "
                         "requests returned (each slot's output region, as "
                         "float32) to DIR/output0.npy")
    ap.add_argument("--full", action="store_true",
                    help="also run the measurements beyond the headline "
                         "figure (none at present: a plain run already does "
                         "only set-up, warmup and the timed steps)")
    args = ap.parse_args()

    import torch

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    distributed = world > 1

    if not torch.cuda.is_available():
        print(json.dumps({"error": "no HIP device available"}))
        return 1

    torch.cuda.set_device(local_rank)
    from client_amd.parallel import (
        OverlappedBroadcaster,
        PeerScatterBroadcaster,
        aggregate_max,
        init_distributed,
    )

    init_distributed("nccl" if distributed else None)
    if distributed:
        import torch.distributed as dist

    import client_amd.grpc as grpcclient
    import client_amd.utils.hip_shared_memory as hipshm

    server_args = [] if args.no_dynamic_batching else [
        "--dynamic-batching",
        "--preferred-batch-size", str(args.preferred_batch_size),
        "--max-queue-delay-us", "400",
    ]
    # stagger the 8 server spawns a little so torch/MIOpen cold-start
    # page-ins don't all land at once (ready window is 300 s)
    if distributed and args.stagger_s > 0:
        time.sleep(local_rank * args.stagger_s)
    server_proc, port = start_server(local_rank, 8101 + local_rank,
                                     server_args, seed=args.seed)
    try:
        client = grpcclient.InferenceServerClient(f"127.0.0.1:{port}")
        for _ in range(240):
            try:
                if client.is_server_ready():
                    break
            except Exception:
                pass
            time.sleep(0.25)

        # per-slot region pairs (bf16 in HBM3E)
        in_elems = int(np.prod(IN_SHAPE))
        out_elems = int(np.prod(OUT_SHAPE))
        slots = []
        for s in range(args.concurrency):
            in_r = hipshm.create_shared_memory_region(
                f"bench_in_{s}", in_elems * 2, local_rank
            )
            out_r = hipshm.create_shared_memory_region(
                f"bench_out_{s}", out_elems * 2, local_rank
            )
            client.register_cuda_shared_memory(
                f"bench_in_{s}", hipshm.get_raw_handle_bytes(in_r), local_rank,
                in_elems * 2,
            )
            client.register_cuda_shared_memory(
                f"bench_out_{s}", hipshm.get_raw_handle_bytes(out_r),
                local_rank, out_elems * 2,
            )
            inp = grpcclient.InferInput("INPUT0", list(IN_SHAPE), "BF16")
            inp.set_shared_memory(f"bench_in_{s}", in_elems * 2)
            out = grpcclient.InferRequestedOutput("OUTPUT0")
            out.set_shared_memory(f"bench_out_{s}", out_elems * 2)
            slots.append({"in": in_r, "out": out_r, "inputs": [inp],
                          "outputs": [out]})

        # synthetic fp32 input, packed on-device to bf16
        host_x = np.random.default_rng(args.seed).random(
            IN_SHAPE, dtype=np.float32)
        for slot in slots:
            hipshm.set_shared_memory_region_cast(slot["in"], host_x, "BF16")

        # world>1 fan-out: ping-pong staging regions so pack(n+1) into
        # one buffer overlaps the broadcast of the other on a side
        # stream (event-ordered; request issue gated on the bcast event
        # only — no per-step global sync). Step n's requests read
        # bench_bc{n%2}; step n+1's pack+bcast run during step n's
        # serving.
        broadcaster = None
        pp_inputs = None
        if distributed:
            pp_regions = []
            pp_inputs = []
            for b in range(2):
                r = hipshm.create_shared_memory_region(
                    f"bench_bc{b}", in_elems * 2, local_rank
                )
                client.register_cuda_shared_memory(
                    f"bench_bc{b}", hipshm.get_raw_handle_bytes(r),
                    local_rank, in_elems * 2,
                )
                hipshm.set_shared_memory_region_cast(r, host_x, "BF16")
                inp = grpcclient.InferInput("INPUT0", list(IN_SHAPE), "BF16")
                inp.set_shared_memory(f"bench_bc{b}", in_elems * 2)
                pp_regions.append(r)
                pp_inputs.append([inp])

            def pack_fn(buf_idx):
                # enqueues h2d + CDNA4 cast on hip_runtime stream 0;
                # the broadcaster orders the collective after it by
                # event
                hipshm.set_shared_memory_region_cast(
                    pp_regions[buf_idx], host_x, "BF16", sync=False
                )

            if args.fanout == "p2p":
                broadcaster = PeerScatterBroadcaster(
                    pp_regions,
                    in_elems * 2,  # per-buffer scatter size
                    src=0,
                )
            else:
                broadcaster = OverlappedBroadcaster(
                    pp_regions, IN_SHAPE, "BF16", src=0
                )

        latencies = []
        lat_lock = threading.Lock()
        step_no = [0]

        def run_step(record=False):
            """(gate on bcast n) -> enqueue pack+bcast n+1 -> serve step
            n (closed loop, reqs_per_step requests at the configured
            concurrency)."""
            n = step_no[0]
            step_no[0] += 1
            if distributed:
                broadcaster.wait_ready()
                broadcaster.stage_and_broadcast((n + 1) % 2, pack_fn)
                step_inputs = pp_inputs[n % 2]
            else:
                hipshm.set_shared_memory_region_cast(
                    slots[0]["in"], host_x, "BF16", sync=True
                )
                step_inputs = None
            # dispatcher model: the main thread issues every request,
            # bounded by a concurrency semaphore; gRPC completion
            # callbacks only record + release (never issue RPCs from
            # completion threads).
            sem = threading.Semaphore(args.concurrency)
            errors = []

            def issue_one(slot_idx):
                slot = slots[slot_idx % len(slots)]
                t0 = time.monotonic_ns()

                def cb(result, error):
                    if error is not None:
                        errors.append(error)
                    elif record:
                        with lat_lock:
                            latencies.append(time.monotonic_ns() - t0)
                    sem.release()

                client.async_infer(
                    "resnet50",
                    step_inputs if step_inputs is not None else slot["inputs"],
                    callback=cb,
                    outputs=slot["outputs"],
                )

            for i in range(args.reqs_per_step):
                if not sem.acquire(timeout=300):
                    raise SystemExit("step timed out (issue)")
                if errors:
                    raise SystemExit(f"infer error: {errors[0]}")
                issue_one(i)
            # drain
            for _ in range(args.concurrency):
                if not sem.acquire(timeout=300):
                    raise SystemExit("step timed out (drain)")
            for _ in range(args.concurrency):
                sem.release()
            if errors:
                raise SystemExit(f"infer error: {errors[0]}")

        # prologue: stage+broadcast buffer 0 so step 0 has data
        if distributed:
            broadcaster.stage_and_broadcast(0, pack_fn)

        # warmup
        for _ in range(args.warmup):
            run_step(record=False)

        # timed region
        if distributed:
            import torch.distributed as dist

            dist.barrier()
        torch.cuda.synchronize()
        t_start = time.monotonic()
        for _ in range(args.steps):
            run_step(record=True)
        torch.cuda.synchronize()
        if distributed:
            dist.barrier()
        t_end = time.monotonic()
        elapsed = t_end - t_start

        # max elapsed over ranks -> whole-job throughput
        elapsed = aggregate_max(elapsed, device="cuda")

        total_requests = args.steps * args.reqs_per_step * world
        total_inferences = total_requests * BATCH
        value = total_inferences / elapsed
        ms_per_step = elapsed / args.steps * 1000.0

        lat_sorted = sorted(latencies)

        def pct(q):
            if not lat_sorted:
                return 0
            return lat_sorted[min(len(lat_sorted) - 1,
                                  int(round(q / 100 * (len(lat_sorted) - 1))))]

        # sanity: output region has live finite data
        logits = hipshm.get_contents_cast(slots[0]["out"], "BF16",
                                          list(OUT_SHAPE))
        assert np.all(np.isfinite(logits)), "non-finite output"

        if args.dump_outputs and rank == 0:
            # a step issues request i into slot i % concurrency, so after
            # the last step these slots hold that step's results
            used = min(args.reqs_per_step, len(slots))
            dumped = np.stack([
                np.asarray(
                    hipshm.get_contents_cast(slot["out"], "BF16",
                                             list(OUT_SHAPE)),
                    dtype=np.float32,
                )
                for slot in slots[:used]
            ])
            os.makedirs(args.dump_outputs, exist_ok=True)
            np.save(os.path.join(args.dump_outputs, "output0.npy"), dumped)

        if distributed:
            fanout_desc = (
                "RCCL tree bcast over xGMI, side-stream overlapped with "
                "next step's pack (hipEvent-ordered, no per-step global "
                "sync)" if args.fanout == "rccl"
                else "7-link hipMemcpyPeerAsync direct scatter over xGMI, "
                     "overlapped with serving"
            )
            bc = broadcaster.bcast_ms[-args.steps:]
            bcast_stats = {
                "mean_ms": round(float(np.mean(bc)), 4) if bc else None,
                "max_ms": round(float(np.max(bc)), 4) if bc else None,
                "timed_from": ("hipEvents on the side stream"
                               if args.fanout == "rccl"
                               else "host clock around scatter+signal"),
            }
        else:
            fanout_desc = "single GPU (no fan-out executed)"
            bcast_stats = None

        if rank == 0:
            print(json.dumps({
                "metric": "perf_analyzer inferences/sec + p99 latency, "
                          "ResNet50 bs=8 HIP-shm at 1/2/4/8 GPU",
                "value": round(value, 2),
                "unit": "inferences/sec",
                "n_gpus": world,
                "steps": args.steps,
                "warmup": args.warmup,
                "ms_per_step": round(ms_per_step, 3),
                "higher_is_better": True,
                "scaling": "weak",
                "vs_baseline": None,
                "dtype": "bf16",
                "data": "synthetic",
                "config": {
                    "model": "resnet50",
                    "global_batch": BATCH * args.reqs_per_step * world,
                    "batch_size": BATCH,
                    "seq_len": None,
                    "parallelism": f"replicated-serving x{world}, one gRPC "
                                   f"client+server pair per GPU, HIP-IPC shm "
                                   f"I/O, fan-out: {fanout_desc}",
                    "bcast": bcast_stats,
                    "concurrency": args.concurrency,
                    "reqs_per_step": args.reqs_per_step,
                    "requests_per_sec": round(total_requests / elapsed, 2),
                    "latency_ms": {
                        "p50": round(pct(50) / 1e6, 3),
                        "p90": round(pct(90) / 1e6, 3),
                        "p99": round(pct(99) / 1e6, 3),
                    },
                },
            }))

        for slot in slots:
            hipshm.destroy_shared_memory_region(slot["in"])
            hipshm.destroy_shared_memory_region(slot["out"])
        if distributed:
            for r in pp_regions:
                hipshm.destroy_shared_memory_region(r)
        client.close()
        if distributed:
            dist.destroy_process_group()
        return 0
    finally:
        server_proc.terminate()
        try:
            server_proc.wait(timeout=10)
        except subprocess.TimeoutExpired:
            server_proc.kill()


if __name__ == "__main__":
    sys.exit(main())
