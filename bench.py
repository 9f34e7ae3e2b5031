#!/usr/bin/env python
"""bench.py — headline benchmark of the bonnie-32 rasterizer hot path on MI355X.

One step = one whole frame of the hot path over a synthetic scene whose inputs are already resident in HBM:
Framebuffer::clear + render_mesh_15 (vertex transform + snap, cull/setup, painter's visibility, tile binning, textured
RGB555-dither fill) and, for N > 1, the gather of the screen bands to rank 0.
Workload at N = 1: BASELINE.json configs[2] "C3" — 2560x1920, 1M-triangle synthetic scene, 8-bit 256x256 atlas.
N > 1 (config C4): one process per GPU, the frame sharded by screen bands; the exchange step is the PRODUCT's own, through the C ABI
(--transport shm: band ranks store their rows straight into rank 0's framebuffer over a HIP IPC mapping, ordered by device-side epoch
words; rccl: b32_gather_bands_rccl; torch: torch.distributed gather) -- checked against the torch-gathered frame before anything is timed,
with a fallback the line reports (`transport`).

Prints ONE JSON line on rank 0 (see the driver contract).  A plain run sets up, warms up, times exactly --steps steps and reports
metric / value / unit / higher_is_better / dtype / ms_per_step (+ the Mpixels/s of the same steps and the run's configuration).
With --full the line also holds
  frame_sha256   the timed frame's SHA-256, checked against tests/golden/hashes.json
  roofline       dominant kernel vs the 8 TB/s HBM peak (HIP events on the kernel's own stream, inside the timed region)
  cpu_baseline   the CPU port of the reference (oracle/, release-profile build, 1 thread) timed on this box's host cores
  cpu_all_cores  the same port threaded (transform split by vertex range, draw split by row band)
  configs        (N = 1) the other BASELINE configs -- C1, C2, C5 -- and C3 with a transparent pass, each with ms/frame, Mtri/s, Mpix/s, frame-level roofline
                 fraction and a framebuffer SHA-256 checked against tests/golden/hashes.json
  protocol       SURVEY 8d extras: median of the per-step times, output-pixel rate, H2D of the scene, D2H of the frame
  weak_series    (N > 1; also without --full when --weak-series is given) the weak-scaling point of SURVEY 8e

--dump-outputs DIR writes what the last timed step computed, in float32 / float64 .npy files (under 64 MB in all):
  frame.npy            (H, W, 4) RGBA8 framebuffer as float32, when it fits; otherwise
  frame_sample.npy     (2^21, 4) float32: the pixels of a fixed seeded sample of pixel indices (sorted), and
  frame_row_sums.npy   (H, 4) float64: per-row sums of every channel (every pixel of the frame contributes)
  timings.npy          float64 [triangles_drawn, fragments, tile_pairs] of the RasterTimings the frame returned
"""
import argparse
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")     # (dmabuf IPC: what the shared-framebuffer transport's hipIpcGetMemHandle / RCCL need on this host driver)
EVENT_STRIDE = int(os.environ.get("B32_BENCH_EVENT_STRIDE", "8"))        # HIP events around the dominant kernel on every 8th step of the timed region
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0   # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec


def csrc_digest():
    """Digest of the library's sources and flags (bonnie-32_amd/build.py): identifies the build a measurement belongs to."""
    from bonnie32_amd import build as B
    return B.csrc_digest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--config", default="C3", help="scene config of bonnie32_amd.scenegen (C1,C2,C3,C5)")
    ap.add_argument("--tris", type=int, default=None)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-configs", action="store_true", help="skip the C1 / C2 / C5 side measurements (profiling runs)")
    ap.add_argument("--cpu-seconds", type=float, default=12.0)
    ap.add_argument("--routes-off", type=lambda v: int(v, 0), default=0,
                    help="B32_ROUTE_* bits to switch off for the whole run (A/B of one route under the profiler; 0 = the library's defaults)")
    ap.add_argument("--check", action="store_true", help="also verify the final frame against the oracle (slow at C3)")
    ap.add_argument("--no-pipeline", action="store_true",
                    help="one stream only: no setup kernel of the next frame beside the fill of the current one (b32_set_routes B32_ROUTE_PIPELINE; "
                         "profiling runs that want kernel durations without overlap)")
    ap.add_argument("--weak-series", action="store_true",
                    help="also time the weak-scaling point of SURVEY 8e (N x 125 k tris on the same frame); always on for N > 1 with --full")
    ap.add_argument("--sync-gather", action="store_true",
                    help="N > 1: gather every frame before the next one starts (default: frames alternate between two framebuffers and the "
                         "gather of one overlaps the rendering of the next, after a run-time self-check against the synchronous frame)")
    ap.add_argument("--pipeline-debug", action="store_true",
                    help="with --dist-backend gloo: run the overlapped-gather logic too (band rows staged through the host)")
    ap.add_argument("--transport", default="shm", choices=["shm", "rccl", "torch"],
                    help="N > 1: how the band rows reach rank 0.  shm (default) = the library's shared-framebuffer transport (b32_band_export / _import, "
                         "device-side epoch words: band ranks store their rows straight into rank 0's HBM); rccl = b32_gather_bands_rccl (grouped "
                         "ncclSend / ncclRecv on the frame's stream, communicator from b32_rccl_comm_create); torch = torch.distributed gather "
                         "(bonnie32_amd.parallel).  shm / rccl are what a host that only speaks the C ABI calls; either falls back to torch -- and the "
                         "line says so -- when its set-up or its run-time self-check against the torch-gathered frame fails")
    ap.add_argument("--dist-backend", default="nccl", choices=["nccl", "gloo"],
                    help="nccl = RCCL over xGMI (default). gloo = debug only: ranks may share one GPU, band rows are staged through the host")
    ap.add_argument("--full", action="store_true",
                    help="also measure and check everything beside the headline: frame hash, protocol extras, per-kernel passes and roofline, "
                         "CPU baselines, the other configs, the weak-scaling point at N > 1 (off: the headline steps only)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's framebuffer and RasterTimings to DIR/*.npy (rank 0)")
    args = ap.parse_args()

    import numpy as np
    import torch
    import torch.distributed as dist

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus and world > 1:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: the rasterizer has no CPU path")
    if args.dist_backend == "gloo":
        local_rank = local_rank % max(torch.cuda.device_count(), 1)
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if args.dist_backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group("gloo")

    import __graft_entry__ as g
    if rank == 0:
        g.build()
    if world > 1:
        dist.barrier()
    from bonnie32_amd import rasterizer as R, scenegen, parallel, abi, exchange as X
    build_digest = abi.check_build_digest()      # refuses a library that was not compiled from this tree's sources
    HASHES = json.load(open(os.path.join(ROOT, "tests", "golden", "hashes.json")))

    sc = scenegen.make_scene(args.config, n_tris=args.tris)
    W, H, NF = sc.width, sc.height, sc.n_tris

    ctx = R.Context(local_rank)
    ctx.set_async_depth(1)      # frames back to back without a host synchronisation (static camera, capacities settled by the warm-up
                                # frames); a frame dropped for lack of buffer space would be REPORTED by finish(), never silent
    if args.no_pipeline or args.routes_off:
        ctx.set_routes((R.Context.ROUTE_PIPELINE if args.no_pipeline else 0) | args.routes_off)
    # one explicit stream for everything of this rank: the rasterizer's kernels, torch's copies and the RCCL gather are ordered by it
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(stream)
    ctx.set_stream(stream.cuda_stream)
    frame = torch.zeros(W * H * 4, dtype=torch.uint8, device=dev)       # the Framebuffer's pixels, in HBM
    fb = R.Framebuffer.__new__(R.Framebuffer)
    fb.ctx = ctx
    fb.bind_device(frame.data_ptr(), W, H)
    y0, y1 = parallel.band_rows(H, world, rank)
    fb.set_band(y0, y1)
    # inputs resident in HBM before the timed region (index atlas + CLUT are expanded on the device); the upload is timed on its own
    torch.cuda.synchronize(dev)
    u0 = time.perf_counter()
    rs = R.ResidentScene(fb, sc.vertices, sc.faces, indexed_textures=sc.indexed_textures)
    torch.cuda.synchronize(dev)
    h2d_ms = (time.perf_counter() - u0) * 1e3
    h2d_bytes = sc.vertices.nbytes + sc.faces.nbytes + sum(t.indices.nbytes + t.clut.nbytes for t in sc.indexed_textures)

    ex = None       # N > 1: the exchange step behind the C ABI (bonnie32_amd.exchange), once its self-check has passed; None = torch.distributed

    def torch_gather():
        if args.dist_backend == "nccl":
            parallel.gather_bands(frame, W, H, world, rank)
        else:       # debug: same gather logic on a host copy
            host = frame.cpu()
            parallel.gather_bands(host, W, H, world, rank)
            if rank == 0:
                frame.copy_(host)

    def draw(rsx, scene, first=False):
        """One step of any resident scene: [exchange: begin] clear + render_mesh_15 [exchange: end | torch gather]"""
        if ex is not None:
            ex.begin()
        fb.clear(scene.clear_color)
        if first:
            rsx.render_async(scene.camera, scene.settings, scene.fog)
        else:
            rsx.render_async()
        if ex is not None:
            ex.end()
        elif world > 1:
            torch_gather()

    def step(first=False):
        draw(rs, sc, first)

    ctx.set_fragment_counting(1)          # warmup frames count the reference's pixel stores exactly (Mpixels/s numerator)
    # warmup (also settles buffer capacities: finish() grows the pair buffers if the first frame overflowed them)
    step(first=True)
    tm = rs.finish()
    for _ in range(max(args.warmup - 1, 0)):
        step()
    tm = rs.finish()

    def sync_all():
        torch.cuda.synchronize(dev)
        if world > 1:
            dist.barrier()
            torch.cuda.synchronize(dev)

    exact_fragments = tm.fragments        # counted exactly during warmup (fragment counting on)
    ctx.set_fragment_counting(0)          # instrumentation off for the timed region (identical framebuffer)
    step(); rs.finish()

    # ---- N > 1: the exchange step through the product's own boundary.  The torch gather above has assembled the
    # reference frame on rank 0; the requested C-ABI transport is set up, the root's framebuffer is poisoned, two frames are drawn
    # through the transport and the root's frame must equal the reference (a band that never arrived leaves poison, a band read too
    # early leaves a half-drawn one) with no wait timed out.  Every rank takes part in both agreement rounds whatever happened to it.
    rdev = dev if args.dist_backend == "nccl" else torch.device("cpu")

    def all_agree(ok):
        flag = torch.tensor([1 if ok else 0], dtype=torch.int32, device=rdev)
        dist.all_reduce(flag, op=dist.ReduceOp.MIN)
        return bool(flag.item())

    transport = {"requested": args.transport if world > 1 else None, "used": "torch" if world > 1 else None, "fallback_reason": None, "timeouts": None,
                 "self_check": None}
    if world > 1 and args.transport != "torch":
        def bcast(payload):
            box = [payload]
            dist.broadcast_object_list(box, src=0)
            return box[0]
        torch.cuda.synchronize(dev)
        ref = frame.cpu().numpy().copy() if rank == 0 else None
        cand, why = None, None
        try:
            if args.transport == "shm":
                cand = X.SharedFramebufferExchange(ctx, W, H, rank, world, bcast)
                fb.width, fb.height = W, H
            else:
                cand = X.RcclExchange(ctx, W, H, rank, world, bcast)
            fb.set_band(y0, y1)
        except Exception as e:                                    # noqa: BLE001
            why = f"set-up on rank {rank}: {e!r}"
        ok = all_agree(why is None)
        if ok:
            try:
                if rank == 0:
                    fb.upload(np.full(W * H * 4, 0xAB, np.uint8))
                dist.barrier()
                ex = cand
                for i in range(2):
                    step(first=(i == 0))
                rs.finish()
                torch.cuda.synchronize(dev)
                if rank == 0 and not np.array_equal(fb.pixels, ref):
                    why = "self-check: the frame assembled through the transport differs from the torch-gathered frame"
                if ex.timeouts():
                    why = f"self-check: {ex.timeouts()} exchange waits timed out"
            except Exception as e:                                # noqa: BLE001
                why = f"self-check on rank {rank}: {e!r}"
            ok = all_agree(why is None)
        if ok:
            transport.update(used=cand.name, self_check="passed")
        else:
            reasons = [None] * world
            dist.all_gather_object(reasons, why)
            transport.update(fallback_reason="; ".join(r for r in reasons if r) or "another rank failed", self_check="failed")
            if rank == 0:
                print(f"# transport {args.transport} unavailable ({transport['fallback_reason']}): timing the torch.distributed gather", file=sys.stderr)
            ex = None
            try:
                if cand is not None:
                    cand.close()
            except Exception:                                     # noqa: BLE001
                pass
            try:
                ctx.finish()
            except Exception:                                     # noqa: BLE001 -- (a band timeout of the failed attempt is not this run's error)
                pass
            fb.bind_device(frame.data_ptr(), W, H)
            fb.set_band(y0, y1)
            step(first=True); rs.finish()

    # ---- N > 1: overlap the band gather with the next frame.  Frames alternate between two framebuffers (two contexts on the same
    # stream, each with the scene resident); the gather of frame i is asynchronous (RCCL's own stream, started after frame i's kernels)
    # and is only waited for when its buffer is about to be redrawn, two frames later.  Every frame is still cleared, rendered and
    # gathered in full.  Guarded by a run-time self-check: pipelined frames must equal the synchronous frame on rank 0, on every
    # rank's agreement, otherwise the synchronous path is timed.
    sets = [(fb, rs, frame)]
    pending = [None, None]
    pipelined = False

    def make_second_set():
        ctx2 = R.Context(local_rank)
        ctx2.set_async_depth(1)
        ctx2.set_stream(stream.cuda_stream)
        frame2 = torch.zeros_like(frame)
        fb2 = R.Framebuffer.__new__(R.Framebuffer)
        fb2.ctx = ctx2
        fb2.bind_device(frame2.data_ptr(), W, H)
        fb2.set_band(y0, y1)
        rs2 = R.ResidentScene(fb2, sc.vertices, sc.faces, indexed_textures=sc.indexed_textures)
        return fb2, rs2, frame2

    def pstep(i, ssets, scene, first=False):
        k = i % len(ssets)
        fbk, rsk, frk = ssets[k]
        if pending[k] is not None:                      # this buffer's previous frame must have left before it is redrawn
            pending[k][0].wait(); pending[k] = None
        fbk.clear(scene.clear_color)
        if first:
            rsk.render_async(scene.camera, scene.settings, scene.fog)
        else:
            rsk.render_async()
        if args.dist_backend == "nccl":
            pending[k] = parallel.gather_bands_async(frk, W, H, world, rank)
        else:               # debug: the same alternation and waits, rows staged through a host copy (gloo has no device gather)
            host = frk.cpu()
            work, keep = parallel.gather_bands_async(host, W, H, world, rank)

            class _HostWait:
                def wait(self, work=work, host=host, frk=frk):
                    work.wait()
                    if rank == 0:
                        frk.copy_(host)
            pending[k] = (_HostWait(), keep)

    def pdrain():
        for k in range(2):
            if pending[k] is not None:
                pending[k][0].wait(); pending[k] = None

    if world > 1 and ex is None and (args.dist_backend == "nccl" or args.pipeline_debug) and not args.sync_gather and H % world == 0:
        ok = 1
        try:
            sets.append(make_second_set())
            torch.cuda.synchronize(dev)
            ref = frame.clone() if rank == 0 else None            # the synchronous frame (assembled by the last step())
            for i in range(4):
                pstep(i, sets, sc, first=(i < 2))
            pdrain()
            sets[0][1].finish(); sets[1][1].finish()
            torch.cuda.synchronize(dev)
            if rank == 0 and not (torch.equal(sets[0][2], ref) and torch.equal(sets[1][2], ref)):
                ok = 0
        except Exception as e:                                    # noqa: BLE001 -- any failure means: time the synchronous path
            print(f"# rank {rank}: pipelined gather unavailable ({e!r}), timing the synchronous path", file=sys.stderr)
            ok = 0
        flag = torch.tensor([ok], dtype=torch.int32, device=dev if args.dist_backend == "nccl" else torch.device("cpu"))
        dist.all_reduce(flag, op=dist.ReduceOp.MIN)
        pipelined = bool(flag.item())
        if not pipelined:
            pending[0] = pending[1] = None
            sets = sets[:1]
            step(); rs.finish()

    def max_over_ranks(seconds):
        t = torch.tensor([seconds], dtype=torch.float64, device=rdev)
        if world > 1:
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item())

    # ---- N > 1 only: the frame LATENCY beside the pipelined throughput -- K frames, each gathered before the next one starts
    sync_ms = None
    if pipelined and args.full:
        sync_all()
        s0 = time.perf_counter()
        for _ in range(args.steps):
            step()
        sync_all()
        sync_ms = max_over_ranks(time.perf_counter() - s0) / args.steps * 1e3
        rs.finish()

    # ---- timed region: exactly K steps, HIP events around the dominant kernel on the stream it runs on
    # (events around k_cover on every 8th frame: an event pair on every frame costs the stream ~10 % -- consecutive frames' kernels no
    # longer run back to back -- and the sampled launches are launches of the timed region all the same)
    ctx.set_profiling_stride(EVENT_STRIDE)
    ctx.set_profiling(1)
    # The W warm-up steps above settle buffer capacities; they do not bring the GPU to its sustained state: the first ~150 frames after
    # an idle phase run 3-5 % slower than the following ones (measured: 20-step regions of 0.138, 0.135, 0.133 ms per step back to back,
    # 0.131 from the fourth on; tools/step_probe2.py).  A further untimed run of frames, reported in `protocol`, puts the timed region
    # into the state a renderer is in after its first tenth of a second.
    SUSTAIN_FRAMES = 160
    import gc
    gc.collect(); gc.disable()                 # (no collector pause inside the ~3 ms timed region -- nor an idle GPU right before it)
    for _ in range(SUSTAIN_FRAMES):
        step()
    rs.finish()
    sync_all()
    pipelined_before = ctx.route_counts().get("pipelined", 0)
    t0 = time.perf_counter()
    if pipelined:
        for i in range(args.steps):
            pstep(i, sets, sc)
        pdrain()
    else:
        for _ in range(args.steps):
            step()
    torch.cuda.synchronize(dev)
    if world > 1:
        dist.barrier()
        torch.cuda.synchronize(dev)
    t1 = time.perf_counter()
    gc.enable()
    tm = rs.finish()
    if pipelined:
        sets[1][1].finish()
    if ex is not None:
        transport["timeouts"] = ex.timeouts()       # (must be 0: a wait that gave up means a frame with stale rows was timed)
    cover_ms_timed = ctx.last_kernel_times().get("cover", None)     # HIP events around k_cover on the stream it runs on (overlapped frames)
    ctx.set_profiling(0)
    ctx.set_profiling_stride(1)
    pipelined_frames = ctx.route_counts().get("pipelined", 0) - pipelined_before      # frames of the timed region only

    if args.dump_outputs and rank == 0:
        # what the last timed step handed its caller: the framebuffer (the set the last step drew into) and its RasterTimings
        last_fb = sets[(args.steps - 1) % len(sets)][0] if pipelined else fb
        px = last_fb.pixels.reshape(H, W, 4)
        os.makedirs(args.dump_outputs, exist_ok=True)

        def out(name, a):
            np.save(os.path.join(args.dump_outputs, name + ".npy"), a)
        if px.size * 4 <= 48 << 20:
            out("frame", px.astype(np.float32))
        else:
            idx = np.sort(np.random.default_rng(0).choice(W * H, size=1 << 21, replace=False))
            out("frame_sample", px.reshape(W * H, 4)[idx].astype(np.float32))
        out("frame_row_sums", px.sum(axis=1, dtype=np.float64))
        out("timings", np.array([tm.triangles_drawn, tm.fragments, tm.tile_pairs], np.float64))

    frags = torch.tensor([float(exact_fragments)], dtype=torch.float64, device=rdev)
    if world > 1:
        dist.all_reduce(frags, op=dist.ReduceOp.SUM)
    elapsed = max_over_ranks(t1 - t0)
    fragments = int(frags.item())
    ms_per_step = elapsed / args.steps * 1e3

    # ---- SURVEY 8d protocol extras (untimed region): per-step device times -> median; D2H of the finished frame
    per_step = []
    if world == 1 and args.full:
        n_med = max(args.steps, 20)
        evs = [torch.cuda.Event(enable_timing=True) for _ in range(n_med + 1)]
        torch.cuda.synchronize(dev)
        for i in range(n_med):
            evs[i].record(stream)
            step()
        evs[n_med].record(stream)
        rs.finish()
        torch.cuda.synchronize(dev)
        per_step = sorted(evs[i].elapsed_time(evs[i + 1]) for i in range(n_med))
    d0 = time.perf_counter()
    final_host = fb.pixels if rank == 0 and (args.full or args.check) else None      # b32_fb_download: the presenter's copy (game/renderer.rs:179)
    d2h_ms = (time.perf_counter() - d0) * 1e3

    # ---- kernel durations WITHOUT overlap (untimed passes, one stream): in the timed region the next frame's setup kernel runs beside
    # the fill kernel, so an event pair around the fill there measures a shared GPU.  (a) events around the fill kernel of every frame,
    # >= 20 samples; (b) events around every phase; an empty phase ("sort": nothing is launched between its two events on the default
    # path) is what an event pair itself costs.
    cover_ms, cover_samples, phases = None, 0, {}
    shader_clock_ghz, shader_clock_ms = 0.0, 0.0
    if world == 1 and args.full:
        ctx.set_routes(R.Context.ROUTE_PIPELINE | args.routes_off)
        n_iso = min(max(args.steps, 24), 60)
        ctx.set_profiling(1)
        for _ in range(n_iso):
            step()
        rs.finish()
        cover_ms = ctx.last_kernel_times().get("cover", None); cover_samples = n_iso
        shader_clock_ghz, shader_clock_ms = ctx.last_shader_clock()    # measured inside the fill kernel of the pass's last frame (one stream)
        ctx.set_profiling(2)
        for _ in range(20):
            step()
        rs.finish()
        phases = ctx.last_kernel_times()
        ctx.set_profiling(0)
        # single-frame latency: every frame finished (host round trip) before the next is enqueued
        torch.cuda.synchronize(dev)
        l0 = time.perf_counter()
        for _ in range(max(args.steps, 20)):
            step(); rs.finish()
        latency_ms = (time.perf_counter() - l0) / max(args.steps, 20) * 1e3
        # throughput of the same loop on one stream (no two frames in flight), and in the library's default SAFE mode
        # (b32_set_async_depth(0): a large scene's pending frame is settled -- one host synchronisation -- before the next is enqueued)
        torch.cuda.synchronize(dev)
        q0 = time.perf_counter()
        for _ in range(args.steps):
            step()
        torch.cuda.synchronize(dev)
        one_stream_ms = (time.perf_counter() - q0) / args.steps * 1e3
        rs.finish()
        ctx.set_routes((R.Context.ROUTE_PIPELINE if args.no_pipeline else 0) | args.routes_off)
        # (twice: with the framebuffer this run draws into -- a torch tensor bound by b32_fb_bind_device, where a clear settles the pending
        # frame because the tensor can be read behind the library's back -- and with the library's own framebuffer (b32_fb_new, what the
        # drop-in Framebuffer::new gives a host), where a clear of the whole band supersedes the pending frame instead)
        ctx.set_async_depth(0)
        torch.cuda.synchronize(dev)
        q0 = time.perf_counter()
        for _ in range(args.steps):
            step()
        torch.cuda.synchronize(dev)
        safe_bound_ms = (time.perf_counter() - q0) / args.steps * 1e3
        rs.finish()
        own = R.Framebuffer(W, H, ctx)                      # b32_fb_new: the context now draws into its own allocation
        own.set_band(y0, y1)
        for _ in range(3):
            step()
        rs.finish(); torch.cuda.synchronize(dev)
        q0 = time.perf_counter()
        for _ in range(args.steps):
            step()
        torch.cuda.synchronize(dev)
        safe_ms = (time.perf_counter() - q0) / args.steps * 1e3
        rs.finish()
        safe_sha = hashlib.sha256(own.pixels).hexdigest()
        fb.bind_device(frame.data_ptr(), W, H); fb.set_band(y0, y1)
        ctx.set_async_depth(1)
    else:
        cover_ms, cover_samples = cover_ms_timed, (args.steps + EVENT_STRIDE - 1) // EVENT_STRIDE
        latency_ms = one_stream_ms = safe_ms = safe_bound_ms = safe_sha = None

    # ---- weak-scaling point (north_star's >= 0.7 target): N x 125 k triangles on the same 2560x1920 frame, so every
    # rank's band keeps the fragments and binned triangles of the 1-GPU 125 k scene.  Reported beside the headline (which is the
    # fixed C3 scene, i.e. strong scaling, as `metric` states); raw times only, the driver derives efficiencies.
    final_frame = final_host if (args.check and rank == 0) else None      # the C3 frame, before the weak series redraws
    weak = None
    if (world > 1 and args.full) or args.weak_series:
        per_gpu = 125000
        wsc = scenegen.make_scene(args.config, n_tris=per_gpu * world)
        wrs = R.ResidentScene(fb, wsc.vertices, wsc.faces, indexed_textures=wsc.indexed_textures)

        def wstep(first=False):
            draw(wrs, wsc, first)

        wsets = [(fb, wrs, frame)]
        if pipelined:       # the same overlap as the headline: the second framebuffer's context gets the weak scene too
            wsets.append((sets[1][0], R.ResidentScene(sets[1][0], wsc.vertices, wsc.faces, indexed_textures=wsc.indexed_textures), sets[1][2]))
            for i in range(2 + 2 * max(args.warmup - 1, 0)):
                pstep(i, wsets, wsc, first=(i < 2))
            pdrain()
            wsets[0][1].finish(); wsets[1][1].finish()
        else:
            wstep(first=True); wrs.finish()
            for _ in range(max(args.warmup - 1, 0)):
                wstep()
            wrs.finish()
        sync_all()
        w0 = time.perf_counter()
        if pipelined:
            for i in range(args.steps):
                pstep(i, wsets, wsc)
            pdrain()
        else:
            for _ in range(args.steps):
                wstep()
        torch.cuda.synchronize(dev)
        if world > 1:
            dist.barrier()
            torch.cuda.synchronize(dev)
        w1 = time.perf_counter()
        wrs.finish()
        if pipelined:
            wsets[1][1].finish()
        w_ms = max_over_ranks(w1 - w0) / args.steps * 1e3
        # the 1-GPU point of the same series, on rank 0's GPU alone: 125 k triangles, whole frame, no gather
        one_ms = None
        if rank == 0:
            osc = scenegen.make_scene(args.config, n_tris=per_gpu)
            fb.set_band(0, H)
            ors = R.ResidentScene(fb, osc.vertices, osc.faces, indexed_textures=osc.indexed_textures)
            fb.clear(osc.clear_color); ors.render_async(osc.camera, osc.settings, osc.fog); ors.finish()
            for _ in range(max(args.warmup - 1, 0)):
                fb.clear(osc.clear_color); ors.render_async()
            ors.finish(); torch.cuda.synchronize(dev)
            o0 = time.perf_counter()
            for _ in range(args.steps):
                fb.clear(osc.clear_color); ors.render_async()
            ors.finish(); torch.cuda.synchronize(dev)
            one_ms = (time.perf_counter() - o0) / args.steps * 1e3
            fb.set_band(y0, y1)
        if world > 1:
            dist.barrier()
        if rank == 0:
            weak = {"scaling": "weak", "tris_per_gpu": per_gpu, "tris": per_gpu * world, "ms_per_step": round(w_ms, 5),
                    "value": round(per_gpu * world / (w_ms * 1e-3) / 1e6, 3), "unit": "Mtriangles/s",
                    "one_gpu_ms_per_step": round(one_ms, 5), "one_gpu_value": round(per_gpu / (one_ms * 1e-3) / 1e6, 3)}

    # ---- the other BASELINE configs on this GPU (N = 1): C1 and C2 (320x240) and C5 (heavy overdraw), same protocol, frames checked
    # against the committed hashes
    side = None
    if args.full and world == 1 and rank == 0 and not args.no_configs and args.config == "C3" and args.tris is None:
        side = {}
        for name in ("C1", "C2", "C5", "C3:blend"):
            # ("C3:blend": the headline scene with 10 % of its faces in the transparent pass -- ordinary content for the reference,
            # render.rs:2522-2532, 2563-2569 -- so that the ordered pass is tracked by the driver's line too)
            s2 = scenegen.make_scene("C3", variant="blend") if name == "C3:blend" else scenegen.make_scene(name)
            c2 = R.Context(local_rank)
            c2.set_async_depth(1)
            c2.set_stream(stream.cuda_stream)
            f2 = R.Framebuffer(s2.width, s2.height, c2)
            if name == "C3:blend":
                r2 = R.ResidentScene(f2, s2.vertices, s2.faces, s2.textures)
            else:
                r2 = R.ResidentScene(f2, s2.vertices, s2.faces, indexed_textures=s2.indexed_textures)
            c2.set_fragment_counting(1)
            f2.clear(s2.clear_color); r2.render_async(s2.camera, s2.settings, s2.fog)
            tm2 = r2.finish()
            c2.set_fragment_counting(0)
            for _ in range(5):
                f2.clear(s2.clear_color); r2.render_async()
            r2.finish()
            k2 = max(args.steps, 100) * (4 if name in ("C1", "C2") else 1)       # (100 / 400 frames: a 20-frame region is a fifth pipeline fill and drain)
            torch.cuda.synchronize(dev)
            q0 = time.perf_counter()
            for _ in range(k2):
                f2.clear(s2.clear_color); r2.render_async()
            torch.cuda.synchronize(dev)
            ms2 = (time.perf_counter() - q0) / k2 * 1e3
            r2.finish()
            sha = hashlib.sha256(f2.pixels).hexdigest()
            tex2 = sum(t.width * t.height * 2 for t in s2.textures)
            alg2 = 36 * len(s2.vertices) + 20 * s2.n_tris + 16 * tm2.triangles_drawn + 8 * s2.width * s2.height + tex2
            side[name] = {"workload": f"{s2.n_tris} tris @ {s2.width}x{s2.height}", "ms_per_frame": round(ms2, 5), "frames": k2,
                          "mtriangles_per_s": round(s2.n_tris / (ms2 * 1e-3) / 1e6, 2),
                          "mpixels_per_s": round(tm2.fragments / (ms2 * 1e-3) / 1e6, 2),
                          "output_mpixels_per_s": round(s2.width * s2.height / (ms2 * 1e-3) / 1e6, 2),
                          "triangles_drawn": tm2.triangles_drawn, "fragments": tm2.fragments,
                          "frame_algorithmic_bytes": alg2, "frame_frac": round(alg2 / (ms2 * 1e-3) / 1e9 / HBM_PEAK_GBS, 5),
                          "sha256": sha[:16], "bit_exact_vs_committed_hash": sha == HASHES[name]["sha256"] and
                          (tm2.triangles_drawn, tm2.fragments) == (HASHES[name]["triangles_drawn"], HASHES[name]["fragments"])}
            del r2, f2, c2

    if rank == 0:
        mtri = NF / (ms_per_step * 1e-3) / 1e6
        mpix = fragments / (ms_per_step * 1e-3) / 1e6
        # ALGORITHMIC bytes.  Frame: SURVEY 8d B_alg.  Dominant kernel k_cover (coverage + shading of the
        # default fast path), per launch, every input counted once:
        #   per (surface, tile) pair: 4 B surface id + 4 B painter's key + 64 B of the surface record (edges, bbox, uv, flags)
        #   per surface: 16 B more of its record for shading (vertex colours)
        #   per band pixel: 4 B framebuffer write;  + the texture once
        tex_bytes = sum(t.width * t.height * 2 for t in sc.textures)
        alg_frame = 36 * len(sc.vertices) + 20 * NF + 16 * tm.triangles_drawn + 8 * W * H + tex_bytes   # SURVEY 8d B_alg
        roofline = None
        if cover_ms and args.full:
            alg_cover = 72 * tm.tile_pairs + 16 * tm.triangles_drawn + 4 * W * (y1 - y0) + tex_bytes
            ach = alg_cover / (cover_ms * 1e-3) / 1e9
            # HBM traffic of the dominant kernel: PMC counters need rocprofv3 around the process, so this is the per-launch figure of
            # the committed PMC passes -- reported only when those passes were taken from THIS build of the kernels (digest over the
            # kernel sources), null otherwise; `traffic_source` says which
            tj = {}
            tpath = os.path.join(ROOT, "profiles", "pmc_traffic.json")
            if os.path.exists(tpath) and world == 1:
                try:
                    tj = json.load(open(tpath))
                except Exception:                                   # noqa: BLE001
                    tj = {}

            def pmc_entry(kernel):
                e = tj.get(f"{args.config}:{kernel}")
                if not isinstance(e, dict):
                    return None, None, None
                same = e.get("csrc_digest") == csrc_digest()
                src = {"file": e.get("file"), "csrc_digest": e.get("csrc_digest"), "this_build": csrc_digest(), "same_build": same,
                       "measured_in_this_run": False, "stale_bytes": None if same else e.get("bytes")}
                return (e.get("bytes") if same else None), src, (e if same else None)
            traffic, tsrc, ecov = pmc_entry("k_cover")
            # the kernel's REAL bound beside the contractual HBM fraction: VALU issue.  wave_instr = SQ_INSTS_VALU of the committed PMC pass
            # (same build only); a wave64 VALU instruction occupies its SIMD for 4 cycles, 4 SIMDs x n_cu CUs issue in parallel.
            valu = None
            if ecov and ecov.get("valu_wave_instr"):
                n_simd = 4 * torch.cuda.get_device_properties(dev).multi_processor_count
                # shader clock: measured by the kernel itself (cycle counter against the 100 MHz wall clock over workgroup 0's lifetime);
                # issue cost: gfx950 issues add / sub / logic / right shift / mov / f32 add-mul-fma in ~2 cycles per wave64 and everything else
                # (min / max / cvt / cmp / 3-operand integer / multiplies / packed) in ~4 -- measured, profiles/r04_instruction_rates.txt; the
                # fused kernel's hot loops are ~35 % of the first kind (ISA mix), i.e. ~3.3 cycles per instruction; 4 is the upper bound
                clk = shader_clock_ghz if shader_clock_ghz and shader_clock_ghz > 0.5 else ecov.get("shader_clock_ghz", 2.4)
                issue_us = ecov["valu_wave_instr"] / n_simd * 3.3 / (clk * 1e3)
                issue_us_hi = ecov["valu_wave_instr"] / n_simd * 4 / (clk * 1e3)
                valu = {"wave_instr": ecov["valu_wave_instr"], "simds": n_simd, "cycles_per_wave_instr": 3.3, "cycles_per_wave_instr_upper": 4,
                        "clock_ghz": round(clk, 3), "clock_source": "measured in the kernel (b32_last_shader_clock)" if shader_clock_ghz and shader_clock_ghz > 0.5 else "nominal",
                        "issue_peak_us": round(issue_us, 2), "issue_peak_us_upper": round(issue_us_hi, 2), "frac": round(issue_us / (cover_ms * 1e3), 4),
                        "lds_bank_conflict_cycles": ecov.get("lds_bank_conflict"), "wait_any_share": ecov.get("wait_any_share")}
            roofline = {"kernel": "k_cover_plain", "kernel_note": "cover_body<..., P64, PLAIN = 1> under a 112-VGPR cap (b32_fill.hip); `cover` in phases_ms; key `<config>:k_cover` of profiles/pmc_traffic.json",
                        "bound": "hbm", "achieved": round(ach, 2), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                        "frac": round(ach / HBM_PEAK_GBS, 5), "traffic": traffic, "traffic_source": tsrc,
                        "kernel_ms": round(cover_ms, 4), "kernel_ms_samples": cover_samples,
                        "kernel_ms_note": "HIP events around the kernel on its own stream, every frame of an untimed pass on ONE stream (no other kernel beside it)" if world == 1 else "timed region",
                        "kernel_ms_timed_region": round(cover_ms_timed, 4) if cover_ms_timed else None,
                        "kernel_ms_timed_region_samples": (args.steps + EVENT_STRIDE - 1) // EVENT_STRIDE,
                        "kernel_ms_timed_region_note": "same events on every 8th step of the timed region, where the next frame's setup kernel runs beside this kernel",
                        "event_pair_overhead_ms": round(phases.get("sort", 0.0), 4) if phases else None,
                        "algorithmic_bytes": alg_cover, "units": {"tile_pairs": tm.tile_pairs, "surfaces": tm.triangles_drawn, "pixels": W * (y1 - y0)},
                        "valu": valu,
                        "frame_algorithmic_bytes": alg_frame,
                        "frame_frac": round(alg_frame / (ms_per_step * 1e-3) / 1e9 / HBM_PEAK_GBS, 5)}
            # second kernel of the frame, the one nearest the HBM roofline: k_setup.  Algorithmic bytes per launch:
            # 20 B face + 36 B of packed positions per face, 36 B of packed (u, v, rgba) + 96 B of records + 4 B face id per surviving
            # face, 4 B painter's key per face slot, 4 B per (surface, tile) pair appended to a tile list
            if phases.get("setup"):
                alg_setup = (20 + 36 + 4) * NF + (36 + 96 + 4) * tm.triangles_drawn + 4 * tm.tile_pairs
                s_ms = phases["setup"]
                s_traffic, s_src, _ = pmc_entry("k_setup")
                roofline["setup"] = {"kernel": "k_setup", "bound": "hbm", "achieved": round(alg_setup / (s_ms * 1e-3) / 1e9, 2), "peak": HBM_PEAK_GBS,
                                     "unit": "GB/s", "frac": round(alg_setup / (s_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 5), "traffic": s_traffic,
                                     "traffic_source": s_src, "kernel_ms": round(s_ms, 4), "kernel_ms_samples": 20, "algorithmic_bytes": alg_setup,
                                     "traffic_frac_of_peak": round(s_traffic / (s_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4) if s_traffic else None}
        cpu = None
        cpu_all = None
        if args.full and world == 1 and not args.no_cpu_baseline:
            from oracle import oracle as O
            ofb = O.Framebuffer(W, H)
            reps, t_cpu = 0, 0.0
            while t_cpu < args.cpu_seconds and reps < 50:
                ofb.clear(sc.clear_color)
                c0 = time.perf_counter()
                rc, otm = O.render_mesh_15(ofb, sc.vertices, sc.faces, sc.textures, sc.camera, sc.settings, sc.fog, fast=True)
                t_cpu += time.perf_counter() - c0
                reps += 1
            per = t_cpu / reps
            want = HASHES.get(args.config, {}).get("sha256") if args.tris is None else None
            cpu = {"value": round(NF / per / 1e6, 4), "unit": "Mtriangles/s", "cores": 1, "kind": "port",
                   "mpixels_per_s": round(otm.fragments / per / 1e6, 3), "ms_per_frame": round(per * 1e3, 2),
                   "build": "gcc -O3 -flto -ffp-contract=off -msse2 (the reference's release profile, Cargo.toml:52-54; oracle/Makefile: libb32oracle_fast.so)",
                   "frame_identical_to_checker_hash": (hashlib.sha256(ofb.pixels).hexdigest() == want) if want else None,
                   "sample": f"{reps} full frames of the same {args.config} scene ({NF} tris @ {W}x{H}), oracle/b32_oracle.c, 1 thread"}
            # the "fair CPU" variant of SURVEY 8d beside it: the same port threaded inside one process -- the per-vertex transform split
            # by vertex range, cull / setup split by face range with ordered concatenation, a parallel stable merge sort, the draw split
            # by row band (the reference itself is single-threaded); frame asserted identical to the single-core one
            try:
                ncpu = os.cpu_count() or 1
                best = None
                for cand in sorted({max(1, min(c, ncpu, H)) for c in (8, 16, 32, 64, 128, 256)}):
                    afb = O.Framebuffer(W, H)
                    ts = []
                    for _ in range(2):
                        afb.clear(sc.clear_color)
                        a0 = time.perf_counter()
                        O.render_mesh_15(afb, sc.vertices, sc.faces, sc.textures, sc.camera, sc.settings, sc.fog, fast=True, threads=cand)
                        ts.append(time.perf_counter() - a0)
                    if best is None or min(ts) < best[0]:
                        best = (min(ts), afb.pixels.copy(), cand)
                t_all, frame_all, cores = best
                cpu_all = {"value": round(NF / t_all / 1e6, 4), "unit": "Mtriangles/s", "cores": cores, "kind": "port",
                           "mpixels_per_s": round(otm.fragments / t_all / 1e6, 3), "ms_per_frame": round(t_all * 1e3, 2),
                           "identical_to_single_core_frame": bool(np.array_equal(frame_all, ofb.pixels)),
                           "speedup_vs_one_core": round(per / t_all, 2),
                           "sample": f"best of 2 frames of the same scene, {cores} threads in one process (transform by vertex range, cull/setup by face range with "
                                     f"ordered concatenation, parallel stable merge sort, draw by row band; fastest of 8..256 threads on {ncpu} host CPUs), "
                                     f"oracle/b32_oracle.c release-profile build"}
            except Exception as e:                                  # noqa: BLE001 -- an extra, never a reason to lose the bench line
                cpu_all = {"error": repr(e)}
        if args.check:
            from oracle import oracle as O
            cfb = O.Framebuffer(W, H); cfb.clear(sc.clear_color)
            O.render_mesh_15(cfb, sc.vertices, sc.faces, sc.textures, sc.camera, sc.settings, sc.fog)
            got = final_frame
            ok = np.array_equal(got, cfb.pixels)
            print("# parity vs oracle:", "bit-exact" if ok else "MISMATCH", file=sys.stderr)
            if not ok:
                bad = (got.reshape(H, W, 4) != cfb.pixels.reshape(H, W, 4)).any(axis=2)
                rows = np.nonzero(bad.any(axis=1))[0]
                print(f"#   {int(bad.sum())} pixels differ, rows {rows.min()}..{rows.max()} ({len(rows)} rows)", file=sys.stderr)
        line = {
            "metric": "Mtriangles/s + Mpixels/s, 1M-tri synthetic scene @ 2560x1920",
            "value": round(mtri, 3), "unit": "Mtriangles/s",
            "mpixels_per_s": round(mpix, 2),
            "output_mpixels_per_s": round(W * H / (ms_per_step * 1e-3) / 1e6, 2),
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 5), "higher_is_better": True,
            "scaling": "strong", "vs_baseline": None, "dtype": "f32+i32 (exact-order f32 setup/barycentrics, integer snap and RGB555 colour tail)",
            "data": "synthetic",
            "config": {"workload": f"{args.config}: {NF} tris @ {W}x{H}, 256x256 8-bit atlas, affine+snap+RGB555 dither, painter's",
                       "triangles_drawn": tm.triangles_drawn, "fragments": fragments,
                       "parallelism": (f"screen bands x{world}, " + (
                           "shared framebuffer through the C ABI (b32_band_export / _import: band ranks store their rows straight into rank 0's HBM; device-side epoch words, b32_band_publish / _wait_all / _acquire)" if transport["used"] == "shm" else
                           "b32_gather_bands_rccl through the C ABI (grouped ncclSend / ncclRecv on the frame's stream) after every frame" if transport["used"] == "rccl" else
                           "torch.distributed gather " + ("overlapped with the next frame (two framebuffers)" if pipelined else "after every frame"))) if world > 1 else "single GPU"},
            "transport": transport if world > 1 else None,
            "build_digest": build_digest, "csrc_digest": csrc_digest(),     # the loaded library's own digest == the source tree's (checked at start)
        }
        if args.full:
            sha = hashlib.sha256(final_host).hexdigest()
            want = HASHES.get(args.config, {}).get("sha256") if args.tris is None else None
            line.update({
                "frame_sha256": sha[:16], "bit_exact_vs_committed_hash": (sha == want) if want else None,
                "protocol": {"ms_per_step_median": round(per_step[len(per_step) // 2], 5) if per_step else None,
                             "ms_per_step_min": round(per_step[0], 5) if per_step else None,
                             "median_over": len(per_step), "median_note": "HIP events between consecutive steps on the frame's stream (separate pass)",
                             "h2d_ms": round(h2d_ms, 3), "h2d_bytes": h2d_bytes, "d2h_ms": round(d2h_ms, 3), "d2h_bytes": W * H * 4,
                             "sync_gather_ms_per_step": round(sync_ms, 5) if sync_ms is not None else None,
                             "untimed_frames_before_timed_region": SUSTAIN_FRAMES + args.warmup + 1,
                             "async_depth": 1, "frames_in_flight": 1 if args.no_pipeline else 2, "pipelined_frames_in_timed_region": pipelined_frames,
                             "async_note": "timed region: b32_set_async_depth(1), frames enqueued back to back; the setup kernel of frame i+1 runs on the "
                                           "library's second stream beside the fill of frame i (two frame sets); every frame is cleared, set up and drawn in full",
                             "frame_latency_ms": round(latency_ms, 5) if latency_ms else None,
                             "ms_per_step_one_stream": round(one_stream_ms, 5) if one_stream_ms else None,
                             "ms_per_step_safe_mode": round(safe_ms, 5) if safe_ms else None,
                             "ms_per_step_safe_mode_bound_fb": round(safe_bound_ms, 5) if safe_bound_ms else None,
                             "safe_mode_frame_identical": (safe_sha == sha) if safe_sha else None,
                             "safe_mode_note": "b32_set_async_depth(0), the library default.  ms_per_step_safe_mode: the library's own framebuffer (b32_fb_new) -- a clear of the "
                                               "whole band supersedes the pending frame, no host synchronisation per frame; ..._bound_fb: caller-bound memory (b32_fb_bind_device, "
                                               "this run's torch tensor) -- every clear settles the pending frame (one host synchronisation): it can be read behind the library's back"},
                "phases_ms": {k: round(v, 4) for k, v in phases.items()},
                "roofline": roofline,
                "cpu_baseline": cpu,
            })
        if side is not None:
            line["configs"] = side
        if weak is not None:
            line["weak_series"] = weak
        if cpu_all is not None:
            line["cpu_all_cores"] = cpu_all
        print(json.dumps(line))
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
