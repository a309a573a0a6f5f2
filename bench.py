#!/usr/bin/env python3
"""bench.py -- RGB-D frames/sec through the MI355X feature front-end (ORB + LSD/LBD extract + Hamming match).

Contract (driver):  python bench.py --gpus N --steps K --warmup W   (N > 1: launched by torch.distributed.run, one rank per GPU).
One "step" = one pass of the whole hot path over one batch of synthetic frames already resident in HBM:
  ORBextractor::operator()  +  LineSegment::ExtractLineSegment  +  the four tracking matchers of the metric --
  ORBmatcher::SearchByProjection(Frame, local map)   (5000-point local map, config-5 load)
  ORBmatcher::SearchByProjection(Cur, Last)          (motion-model search against the last frame)
  LSDmatcher::SearchByProjection(Frame, map lines)   (500 map lines)
  LSDmatcher::SearchByProjection(Cur, Last)          (the brute-force Hamming kNN (k = 2) of the LBD descriptors + MAD rule)
Workloads (--config, numbering = BASELINE.json configs[] counted from 1):
  2 (default)  configs[1]: 640x480, 1000 ORB + 100 lines, the headline metric; --batch frames in flight per GPU (default 8192: eight region-growing chains per SIMD)
  3            configs[2]: 640x480, 2000 ORB + 200 lines, 8 frames in flight on one GPU
  4            configs[3]: 1280x960, 4000 ORB + 400 lines, batch 64 sharded over 8 GPUs = 8 frames in flight per GPU
Frames are independent, so ranks shard the job with no collective (rgbd_pl_slam_amd.batch.shard = plf_batch_shard; weak scaling:
every rank processes its own frames_in_flight).  Prints ONE JSON line on rank 0.  A plain run does only what the headline needs: it sets up, warms up, times
the steps, dumps (--dump-outputs) and prints.  With --full, at N = 1 the default config also carries the secondary figures, each timed in runs of its own (the
headline step on 32 distinct frames, config 3 as specified, single-frame and tracking-call latency, frames/s against frames in flight, the same step on
natural-image-like frames (`natural`) and on windows of REAL photographs (`real_photos`: tests/golden/real), PCIe-inclusive rate through the product's batch
driver, CPU baseline).
--dump-outputs DIR writes what the last timed step of the headline computed (a fixed seeded sample of its frames) as DIR/<name>.npy: the inputs are seeded, so
two builds run with the same arguments can be compared output for output.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

M_POINTS, M_LINES = 5000, 500
CONFIGS = {   # --config -> (width, height, ORB features, lines, frames in flight per GPU, label)
    2: (640, 480, 1000, 100, 8192, "BASELINE configs[1]: VGA, 1000 ORB feats (8 levels) + 100 lines"),
    3: (640, 480, 2000, 200, 8, "BASELINE configs[2]: VGA, 2000 ORB + 200 lines, 8 frames in flight"),
    4: (1280, 960, 4000, 400, 8, "BASELINE configs[3]: 1280x960, 4000 ORB + 400 lines, batch 64 over 8 GPUs = 8 frames in flight per GPU"),
}
HBM_PEAK_GBS = 8000.0


def algorithmic_bytes(w, h, nfeat, nlines, lam_per_line=80):
    """algorithmic bytes per frame of ORB and of the line pipeline, and of the region-growing stage alone"""
    lw, lh, sp, p0, plast = w, h, 0, w * h, 0
    scale = 1.0
    import numpy as np
    sf = np.float32(1.0)
    for l in range(8):
        if l:
            sf = np.float32(np.float64(sf) * np.float64(np.float32(1.2)))
        inv = np.float32(1.0) / sf
        lw, lh = int(np.rint(np.float32(w) * inv)), int(np.rint(np.float32(h) * inv))
        sp += lw * lh
        plast = lw * lh
    K = nfeat
    b_orb = (sp - plast) + (sp - p0) + sp + 2 * sp + 749 * K + 512 * K + 32 * K + 28 * K
    ps = int(0.64 * p0)
    lam = lam_per_line * nlines
    b_line = (p0 + ps) + 9 * ps + 8 * ps + 6 * ps + 5 * p0 + 252 * lam + 124 * nlines
    return b_orb, b_line, 6 * ps


_STREAM_CACHE = {}


class Pipeline:
    """the device-resident step: both extractors + the four matchers for B frames in flight on one GPU"""

    def __init__(self, w, h, nfeat, nlines, B, device, seed_base, serial=False, line_handles=1, front_wait=True, defer_match=True, distinct=1024, family="polygons"):
        import numpy as np
        import torch
        from rgbd_pl_slam_amd import ORBextractor, LineSegment, Matcher, matchgen
        from rgbd_pl_slam_amd._lib import KP_DTYPE, KL_DTYPE
        from rgbd_pl_slam_amd.synth import synth_batch_parallel
        self.torch, self.B, self.w, self.h, self.nlines = torch, B, w, h, nlines
        self.serial, self.front_wait = serial, front_wait
        self.defer_match = defer_match and not serial
        self.pending = None
        # `distinct` independently seeded frames tiled to the batch (a region-growing launch lasts as long as its slowest chain, so 32
        # distinct images tiled 128 times understate the tail of a diverse stream)
        ndist = min(B, max(1, distinct))
        self.ndist = ndist
        # family "natural": synth.natural_frame (1/f texture + blurred scene + sensor noise) instead of the hard-edged polygon scenes
        self.family = family
        self.h_distinct = synth_batch_parallel(seed_base, ndist, w, h, family=family)
        self.d_img = torch.empty((B, h, w), dtype=torch.uint8, device="cuda")
        self.load_images(ndist)
        self.orb = ORBextractor(nfeatures=nfeat, max_width=w, max_height=h, max_batch=B, device=device)
        # (line_handles 2: two handles used alternately so that the NFA / descriptor tail of batch k overlaps the region growing of batch k+1)
        self.lins = [LineSegment(nlines=nlines, max_width=w, max_height=h, max_batch=B, device=device) for _ in range(max(1, min(2, line_handles)))]
        cap = self.cap = self.orb.capacity

        def bufset():
            z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
            neg = lambda shape: torch.full(shape, -1, dtype=torch.int32, device="cuda")
            return dict(kps=z((B, cap, 7), torch.float32), desc=z((B, cap, 32), torch.uint8), nk=z(B, torch.int32),
                        lines=z((B, nlines, 17), torch.float32), ldesc=z((B, nlines, 32), torch.uint8), leq=z((B, nlines, 3), torch.float64), nl=z(B, torch.int32),
                        match_kp=neg((B, cap)), nm_kp=z(B, torch.int32), match_kp_last=neg((B, cap)), nm_kp_last=z(B, torch.int32),
                        match_ln=neg((B, nlines)), nm_ln=z(B, torch.int32), match_ln_last=neg((B, nlines)), nm_ln_last=z(B, torch.int32))
        # feature / match buffers are double-buffered so that the extraction of step k+1 overlaps the matching of step k
        self.bufs = [bufset(), bufset()]
        self.scale = torch.from_numpy(np.ascontiguousarray(self.orb.GetScaleFactors())).cuda()
        # HIP streams: LSD/LBD on a high-priority stream per line handle (region growing is a serial chain per frame and the long pole), ORB on sA,
        # the matchers on sM.  The two extractors are independent, as the two threads of the PL-SLAM Frame constructor are.
        pa, pb, pm = [int(x) for x in os.environ.get("PLF_BENCH_PRIO", "0,-1,0").split(",")]
        # (one set of streams per process, shared by every Pipeline: torch hands out its pooled streams round-robin and HIP maps them onto a few hardware queues,
        # so the ORB and matcher streams of a LATER pipeline could land on one queue -- the natural-image extras, the tenth pipeline of a run, ran 10 % slower and
        # with region-kernel launches alternating between 210 and 330 ms, which a fresh process never showed: profiles/r05_regions_trace.txt)
        key = (device, pa, pb, pm, len(self.lins))
        if key not in _STREAM_CACHE:
            _STREAM_CACHE[key] = (torch.cuda.Stream(priority=pa), [torch.cuda.Stream(priority=pb) for _ in self.lins], torch.cuda.Stream(priority=pm))
        self.sA, sBs_, sM_ = _STREAM_CACHE[key]
        self.sBs = list(sBs_)
        if serial:
            self.sBs = [self.sA for _ in self.lins]
        self.sM = self.sA if serial else sM_
        # local map / last frame built from the features of frame 0 (so that real matches exist); replicas per GPU
        b0 = self.bufs[0]
        torch.cuda.synchronize()
        self.orb.extract_batch_device(self.d_img, w, h, b0["kps"], b0["desc"], b0["nk"], cap, self.sA.cuda_stream)
        self.lins[0].extract_batch_device(self.d_img, w, h, b0["lines"], b0["ldesc"], b0["leq"], b0["nl"], nlines, self.sBs[0].cuda_stream)
        torch.cuda.synchronize()
        n0 = int(b0["nk"][0]); k0 = np.frombuffer(b0["kps"][0, :n0].cpu().numpy().tobytes(), KP_DTYPE)
        d0 = b0["desc"][0, :n0].cpu().numpy()
        l0n = int(b0["nl"][0]); l0 = np.frombuffer(b0["lines"][0, :l0n].cpu().numpy().tobytes(), KL_DTYPE)
        ld0 = b0["ldesc"][0, :l0n].cpu().numpy()
        dev = lambda d: {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in d.items()}
        self.mp = dev(matchgen.make_local_map(k0, d0, M_POINTS, 1, w=w, h=h))
        self.ml = dev(matchgen.make_map_lines(l0, ld0, M_LINES, 2))
        last, pose = matchgen.make_last_frame(k0, d0, 3, cx=w / 2 - 0.5, cy=h / 2 - 0.5)
        last["keys"] = np.frombuffer(np.ascontiguousarray(last["keys"]).tobytes(), np.uint8).copy()
        self.last = dev(last)
        self.last_ldesc = torch.from_numpy(matchgen.flip_bits(ld0, np.random.default_rng(4), 15)).cuda()
        self.last_has_ml = torch.from_numpy((np.random.default_rng(5).uniform(0, 1, l0n) < 0.8).astype(np.uint8)).cuda()
        bounds = (0.0, 0.0, float(w), float(h))
        self.mats = [Matcher(max_keypoints=cap, max_mappoints=M_POINTS, max_lines=max(nlines, 2), max_batch=B, device=device) for _ in range(2)]
        self.last_view = Matcher.last_view(self.last)
        from rgbd_pl_slam_amd import _lib as L
        # every frame of the batch has its own pose (the motion-model prediction differs per frame) and the poses change from step to step, as in a
        # tracking loop: the pose upload is part of every timed step (one constant array always hit the handle's cache)
        prng = np.random.default_rng(6)
        self.poses = []
        for _ in range(3):
            arr = (L.PosePair * B)()
            jit = prng.normal(0.0, 0.002, (B, 3)).astype(np.float32)
            for f in range(B):
                pf = dict(pose); pf["tcw"] = pose["tcw"] + jit[f]
                arr[f] = Matcher.pose_pair(pf)
            self.poses.append(arr)
        for bs in self.bufs:
            bs["fviews"] = Matcher.view_array([Matcher.frame_view(cap, bs["kps"].data_ptr() + f * cap * 28, bs["desc"].data_ptr() + f * cap * 32, self.scale, bounds,
                                                                  None, bs["nk"].data_ptr() + 4 * f) for f in range(B)])
            bs["lviews"] = Matcher.view_array([Matcher.lineframe_view(nlines, bs["lines"].data_ptr() + f * nlines * 68, bs["ldesc"].data_ptr() + f * nlines * 32,
                                                                      self.scale, bs["nl"].data_ptr() + 4 * f) for f in range(B)])
            bs["match_done"] = None
        self.k = 0

    def load_images(self, ndist):
        """fill the resident batch with the first ndist distinct frames, tiled"""
        import numpy as np
        torch, B = self.torch, self.B
        src = torch.from_numpy(self.h_distinct[:ndist]).cuda()
        for lo in range(0, B, ndist):
            n = min(ndist, B - lo)
            self.d_img[lo:lo + n].copy_(src[:n])
        torch.cuda.synchronize()
        self.ndist_loaded = ndist

    def step(self):
        torch = self.torch
        k = self.k; self.k += 1
        bs = self.bufs[k & 1]
        li = k % len(self.lins)
        sA, sBk, sM, w, h = self.sA, self.sBs[li], self.sM, self.w, self.h
        if bs["match_done"] is not None:           # the matchers of step k-2 read this buffer set
            sA.wait_event(bs["match_done"]); sBk.wait_event(bs["match_done"])
        self.lins[li].extract_batch_device(self.d_img, w, h, bs["lines"], bs["ldesc"], bs["leq"], bs["nl"], self.nlines, sBk.cuda_stream)
        ev_lines = torch.cuda.Event(); ev_lines.record(sBk)
        # ORB starts when the line extractor reaches region growing: that kernel is a latency-bound chain that leaves issue slots idle,
        # whereas the line front stages (blur / resize / gradient / Sobel) are throughput-bound like ORB
        if self.front_wait and not self.serial:
            self.lins[li].wait_front(sA.cuda_stream)
        self.orb.extract_batch_device(self.d_img, w, h, bs["kps"], bs["desc"], bs["nk"], self.cap, sA.cuda_stream)
        ev_orb = torch.cuda.Event(); ev_orb.record(sA)
        if self.defer_match:
            # software pipelining: the matchers of step k are enqueued in step k+1, behind the line extractor's front stages, i.e. they run in the shadow of
            # the NEXT region-growing kernel instead of colliding with the next front stages (flush() issues the last ones)
            prev, self.pending = self.pending, (k, ev_orb, ev_lines)
            if prev is not None:
                self.lins[li].wait_front(sM.cuda_stream)
                self._match(*prev)
            return
        self._match(k, ev_orb, ev_lines)

    def flush(self):
        if self.pending is not None:
            prev, self.pending = self.pending, None
            self._match(*prev)

    def _match(self, k, ev_orb, ev_lines):
        torch = self.torch
        bs = self.bufs[k & 1]
        sM = self.sM
        sM.wait_event(ev_orb)
        with torch.cuda.stream(sM):
            bs["match_kp"].fill_(-1); bs["match_kp_last"].fill_(-1); bs["match_ln"].fill_(-1); bs["match_ln_last"].fill_(-1)
        mat = self.mats[k & 1]
        mat.SearchByProjection(bs["fviews"], self.mp, 3.0, 0.8, bs["match_kp"], self.cap, bs["nm_kp"], sM.cuda_stream)
        mat.SearchByProjectionLastFrameBatch(bs["fviews"], self.last_view, self.poses[k % 3], 7.0, 0, 1, bs["match_kp_last"], self.cap, bs["nm_kp_last"], sM.cuda_stream)
        sM.wait_event(ev_lines)
        mat.SearchLinesByProjection(bs["lviews"], self.ml, 3.0, 0.8, bs["match_ln"], self.nlines, bs["nm_ln"], sM.cuda_stream)
        mat.SearchLinesLastFrameBatch(self.last_ldesc, self.last_has_ml, bs["lviews"], bs["match_ln_last"], self.nlines, bs["nm_ln_last"], sM.cuda_stream)
        bs["match_done"] = torch.cuda.Event(); bs["match_done"].record(sM)

    def match_step(self):
        """BASELINE configs[4]: only the matchers, on the features the last step() left in buffer set 0"""
        bs = self.bufs[0]; sM = self.sM; mat = self.mats[0]
        with self.torch.cuda.stream(sM):
            bs["match_kp"].fill_(-1); bs["match_kp_last"].fill_(-1); bs["match_ln"].fill_(-1); bs["match_ln_last"].fill_(-1)
        mat.SearchByProjection(bs["fviews"], self.mp, 3.0, 0.8, bs["match_kp"], self.cap, bs["nm_kp"], sM.cuda_stream)
        self.mk = getattr(self, "mk", 0) + 1
        mat.SearchByProjectionLastFrameBatch(bs["fviews"], self.last_view, self.poses[self.mk % 3], 7.0, 0, 1, bs["match_kp_last"], self.cap, bs["nm_kp_last"], sM.cuda_stream)
        mat.SearchLinesByProjection(bs["lviews"], self.ml, 3.0, 0.8, bs["match_ln"], self.nlines, bs["nm_ln"], sM.cuda_stream)
        mat.SearchLinesLastFrameBatch(self.last_ldesc, self.last_has_ml, bs["lviews"], bs["match_ln_last"], self.nlines, bs["nm_ln_last"], sM.cuda_stream)

    def check(self):
        # the device-resident calls return before the GPU has run: a capacity overflow would make the step's outputs (and its time) meaningless
        for l in self.lins:
            if l.last_status() != 0:
                raise RuntimeError("line extractor reported status %d for the last batch" % l.last_status())

    def matches_frame0(self):
        b = self.bufs[0]
        return {"points_map": int(b["nm_kp"][0]), "points_last_frame": int(b["nm_kp_last"][0]), "lines_map": int(b["nm_ln"][0]),
                "lines_last_frame_knn": int(b["nm_ln_last"][0]), "keypoints": int(b["nk"][0]), "lines": int(b["nl"][0])}

    def chain_stats(self):
        """min / median / max length of the frames' region-growing chains in the last batch (pixels left marked USED; 0 if it took the speculative schedule)"""
        import numpy as np
        c = self.lins[(self.k - 1) % len(self.lins)].chain_lengths(self.B)
        return {"min": int(c.min()), "median": int(np.median(c)), "max": int(c.max()), "mean": round(float(c.mean()), 1),
                "what": "pixels left USED per frame by LSD region growing = length of the frame's serial chain; the one-wave-per-frame launch lasts as long as the longest"}

    def rect_stats(self):
        """rectangles per frame the last batch handed to the NFA validation"""
        import numpy as np
        c = self.lins[(self.k - 1) % len(self.lins)].rect_counts(self.B)
        return {"min": int(c.min()), "median": int(np.median(c)), "max": int(c.max()), "mean": round(float(c.mean()), 1)}

    def rounds_stats(self):
        """validation rounds of the last few-frames batch (None for the other schedules)"""
        import numpy as np
        rs = self.lins[(self.k - 1) % len(self.lins)].spec_rounds(self.B) if self.B <= 16 else None
        if rs is None:
            return None
        ok = rs[:, 3] == 0
        r = rs[ok, 2]; r = r[r > 0]
        return {"frames": int(len(rs)), "finished_by_serial_commit": int((~ok).sum()), "rounds_to_fixpoint_mean": round(float(r.mean()), 2) if len(r) else None,
                "rounds_to_fixpoint_max": int(r.max()) if len(r) else None}

    def lines_kept(self):
        b = self.bufs[(self.k - 1) & 1]
        return round(float(b["nl"].float().mean()), 1)

    def close(self):
        for o in [self.orb] + self.lins + self.mats:
            o.close()


def timed(pipe, steps, warmup, dist=None):
    torch = pipe.torch
    for _ in range(warmup):
        pipe.step()
    pipe.flush()
    torch.cuda.synchronize()
    for l in pipe.lins:
        l.profile(enable=True, reset=True)
    if dist is not None:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        pipe.step()
    pipe.flush()
    torch.cuda.synchronize()
    if dist is not None:
        dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    reg_ms, reg_launches = 0.0, 0
    for l in pipe.lins:
        ms_, n_ = l.profile(enable=False, reset=True)
        reg_ms += ms_; reg_launches += n_
    pipe.check()
    return elapsed, reg_ms, reg_launches


DUMP_BYTES, DUMP_FRAMES, DUMP_SEED = 64_000_000, 256, 2024


def dump_outputs(pipe, out_dir):
    """`--dump-outputs DIR`: what the last timed step handed its caller, as DIR/<name>.npy, for a fixed seeded sample of the batch's frames (at most
    DUMP_FRAMES and DUMP_BYTES in all; the same frames for the same --batch, so that two builds compare output for output).  Key points + descriptors,
    lines + descriptors + line equations, the four matchers' results and every count.  Entries past a frame's count are padding no caller reads: zeroed
    (matches: -1).  Integers become float32, exactly (key point octave / class_id, line class_id / octave / numOfPixels, descriptor bytes, indices,
    counts); line equations stay float64.  Call it right after timed(), before anything else runs on the pipeline."""
    import numpy as np
    torch = pipe.torch
    bs = pipe.bufs[(pipe.k - 1) & 1]          # (step k wrote buffer set k & 1; flush() ran its matchers and timed() synchronised)
    cap, nl = pipe.cap, pipe.nlines
    per_frame = 4 * (cap * (7 + 32 + 2) + nl * (17 + 32 + 2) + 6) + 8 * (3 * nl + 1)
    n = max(1, min(pipe.B, DUMP_FRAMES, DUMP_BYTES // per_frame))
    idx = np.sort(np.random.default_rng(DUMP_SEED).permutation(pipe.B)[:n])
    sel = torch.from_numpy(idx).to(bs["nk"].device)
    if sel.is_cuda:       # (tests/test_bench_dump.py hands it host tensors)
        torch.cuda.synchronize()
    get = lambda key: bs[key].index_select(0, sel).cpu().numpy()
    nk, nln = get("nk"), get("nl")
    kvalid = np.arange(cap)[None, :] < nk[:, None]
    lvalid = np.arange(nl)[None, :] < nln[:, None]

    def with_ints(a, cols):
        f = a.copy()
        f[..., cols] = a.view(np.int32)[..., cols].astype(np.float32)
        return f

    def masked(a, valid, pad=0):
        a = np.array(a, dtype=np.float64 if a.dtype == np.float64 else np.float32)
        a[~valid] = pad
        return a

    out = {"frame_index": idx.astype(np.float64), "keypoint_count": nk.astype(np.float32), "line_count": nln.astype(np.float32),
           "keypoints": masked(with_ints(get("kps"), [5, 6]), kvalid), "descriptors": masked(get("desc"), kvalid),
           "lines": masked(with_ints(get("lines"), [1, 2, 16]), lvalid), "line_descriptors": masked(get("ldesc"), lvalid),
           "line_equations": masked(get("leq"), lvalid)}
    for name, key, valid in (("points_map", "kp", kvalid), ("points_last_frame", "kp_last", kvalid), ("lines_map", "ln", lvalid),
                             ("lines_last_frame", "ln_last", lvalid)):
        out[name + "_matches"] = masked(get("match_" + key), valid, -1)
        out[name + "_match_count"] = get("nm_" + key).astype(np.float32)
    total = sum(a.nbytes for a in out.values())
    assert total <= DUMP_BYTES, total
    os.makedirs(out_dir, exist_ok=True)
    for name, a in out.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)
    return {"dir": out_dir, "frames": int(n), "of_frames": pipe.B, "bytes": int(total), "arrays": sorted(out)}


def _frame_fn(family):
    from rgbd_pl_slam_amd.synth import synth_frame, natural_frame, photo_frame
    return {"natural": natural_frame, "photo": photo_frame}.get(family, synth_frame)


def single_frame_latency(device, w, h, nfeat, nlines, reps=20, family="polygons"):
    """one frame at a time through the host-memory entry points (ORBextractor::operator(), LineSegment::ExtractLineSegment): what a live
    SLAM loop sees"""
    import numpy as np
    from rgbd_pl_slam_amd import ORBextractor, LineSegment
    from rgbd_pl_slam_amd.synth import synth_frame, natural_frame
    orb = ORBextractor(nfeatures=nfeat, max_width=w, max_height=h, device=device)
    lin = LineSegment(nlines=nlines, max_width=w, max_height=h, device=device)
    imgs = [_frame_fn(family)(7000 + i, w, h) for i in range(4)]
    to, tl = [], []
    for i in range(reps + 3):
        t0 = time.perf_counter(); orb(imgs[i % 4]); t1 = time.perf_counter(); lin.ExtractLineSegment(imgs[i % 4]); t2 = time.perf_counter()
        if i >= 3:
            to.append(t1 - t0); tl.append(t2 - t1)
    orb.close(); lin.close()
    return {"orb_ms_median": round(1e3 * float(np.median(to)), 3), "lsd_lbd_ms_median": round(1e3 * float(np.median(tl)), 3), "frames": reps,
            "what": "one %dx%d frame (%s), host memory in and out, nothing else in flight" % (w, h, family)}


def tracking_call_latency(device, cfg, family="polygons", reps=30):
    """What ONE TrackRGBD call sees of this path (Examples/RGB-D/rgbd_tum.cc:96-116 times the call per frame): both extractors of one frame on two streams, then
    the four tracking matchers, synchronised after every frame -- nothing else in flight, features and matches device-resident."""
    import numpy as np
    import torch
    W, H, NFEAT, NLINES, _, label = CONFIGS[cfg]
    from rgbd_pl_slam_amd.synth import synth_frame, natural_frame
    p = Pipeline(W, H, NFEAT, NLINES, 1, device, 4321, defer_match=False, distinct=1, family=family)
    frames = torch.from_numpy(np.stack([_frame_fn(family)(7000 + i, W, H) for i in range(6)])).cuda()   # (the frames of single_frame_latency)
    for i in range(6):
        p.d_img[0].copy_(frames[i]); p.step()
    torch.cuda.synchronize()
    ts, tm = [], []
    for i in range(reps):
        p.d_img[0].copy_(frames[i % 6]); torch.cuda.synchronize()
        t = time.perf_counter(); p.step(); torch.cuda.synchronize(); ts.append(time.perf_counter() - t)
    for _ in range(reps):
        t = time.perf_counter(); p.match_step(); torch.cuda.synchronize(); tm.append(time.perf_counter() - t)
    m0 = p.matches_frame0()
    p.close()
    return {"extract_and_match_ms_median": round(1e3 * float(np.median(ts)), 3), "matchers_alone_ms_median": round(1e3 * float(np.median(tm)), 3), "frames": reps,
            "keypoints": m0["keypoints"], "lines": m0["lines"], "what": "one %dx%d frame (%s), %d ORB + %d lines, both extractors then the four matchers, synchronised per frame" %
                                                                        (W, H, family, NFEAT, NLINES)}


def reduce_elapsed_max(dist, seconds, device="cuda"):
    """the job lasts as long as its slowest rank: MAX over the ranks of one float (the only reduction on the whole path; nccl = RCCL on the GPU box, gloo in the
    CPU test tests/test_sharding.py)"""
    if dist is None:
        return float(seconds)
    import torch
    t = torch.tensor([seconds], dtype=torch.float64, device=device)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return float(t[0])


def pcie_line(r, elapsed_max, world, n_frames, in_flight, steps, warmup, W, H, label, config):
    """the JSON line of `bench.py --pcie` (rank 0): aggregate frames/s over all ranks from the slowest rank's time"""
    frames = world * n_frames * max(1, steps)
    r = dict(r); r.pop("elapsed_max", None)
    return {
        "metric": "RGB-D frames/sec (ORB+LSD extract + BF-Hamming match) at %dx%d, PCIe-inclusive" % (W, H),
        "value": round(frames / elapsed_max, 2), "unit": "frames/s", "n_gpus": world, "steps": max(1, steps), "warmup": max(1, warmup),
        "ms_per_step": round(1e3 * elapsed_max / max(1, steps), 3), "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "u8/f64",
        "data": "synthetic (pinned host frames, 256 distinct per GPU)",
        "config": {"workload": label + "; host frames in, key points / descriptors / lines / local-map matches out in host memory (plf_batch_extract)",
                   "baseline_config": config, "frames_per_call_per_gpu": n_frames, "frames_in_flight_per_gpu": in_flight,
                   "parallelism": "frames sharded over %d GPU(s) by contiguous blocks, no collective" % world},
        "pcie": {"host_read_GBps_aggregate": round(frames * W * H / elapsed_max / 1e9, 2), "host_read_GBps_per_gpu": round(frames * W * H / elapsed_max / 1e9 / world, 2),
                 "rank0": r}}


def run_pcie(args, dist, rank, local_rank, world, B, W, H, NFEAT, NLINES, label, pcie_fn=None, local_map_fn=None):
    """`bench.py --pcie`: every rank drives ITS GPU through the product's batch driver with host buffers of its own (the worker thread is bound to the GPU's NUMA
    node, where the pinned buffers are then placed); K timed calls of 4 x in-flight frames each between barriers, MAX over the ranks.  pcie_fn / local_map_fn are
    the test seams of tests/test_sharding.py (gloo, no GPU): the rank logic and the JSON assembly run unchanged."""
    in_flight = min(B, 4096)
    n_frames = 4 * in_flight
    if local_map_fn is None:
        def local_map_fn():
            pm = Pipeline(W, H, NFEAT, NLINES, 8, local_rank, 10_000 * rank)   # (only for its local map: built from the features of a synthetic frame)
            mp, ml = pm.mp, pm.ml
            pm.close(); del pm
            return mp, ml
    mp, ml = local_map_fn()
    r = (pcie_fn or pcie_inclusive)(local_rank, W, H, NFEAT, NLINES, n_frames, in_flight, mp, ml, reps=max(1, args.steps), warm=max(1, args.warmup), dist=dist)
    if rank != 0:
        return None
    return pcie_line(r, r["elapsed_max"], world, n_frames, in_flight, args.steps, args.warmup, W, H, label, args.config)


def pcie_inclusive(device, w, h, nfeat, nlines, n_frames, in_flight, mp, ml, reps=2, warm=1, dist=None):
    """host frames in, host features + matches out through the product's batch driver (plf_batch_*): pinned caller buffer, double-buffered
    async H2D / D2H, one worker thread per GPU"""
    import numpy as np
    from rgbd_pl_slam_amd.batch import BatchExtractor, pinned_array, free_pinned
    from rgbd_pl_slam_amd.synth import synth_batch_parallel
    bx = BatchExtractor(nfeatures=nfeat, nlines=nlines, width=w, height=h, frames_in_flight=in_flight, devices=[device], max_mappoints=M_POINTS,
                        max_maplines=M_LINES)
    bx.set_local_map({k: v.cpu().numpy() for k, v in mp.items()}, {k: v.cpu().numpy() for k, v in ml.items()}, bounds=(0.0, 0.0, float(w), float(h)))
    pin = pinned_array((n_frames, h, w))
    nd = min(n_frames, 256)
    distinct = synth_batch_parallel(8000, nd, w, h)
    for i in range(n_frames):
        pin[i] = distinct[i % nd]
    out = bx.alloc_outputs(n_frames)
    for _ in range(warm):
        bx.extract_into(pin[:min(n_frames, 2 * in_flight)], {k: v[:min(n_frames, 2 * in_flight)] for k, v in out.items()})   # warm-up (allocations, tables)
    best, total = None, 0.0
    if dist is not None:
        dist.barrier()
    for _ in range(reps):
        t0 = time.perf_counter()
        bx.extract_into(pin, out)
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
        total += dt
    elapsed_max = reduce_elapsed_max(dist, total)   # the job lasts as long as its slowest rank
    tm = bx.last_timing()
    aff = bx.worker_affinity(0)
    per_worker = [{k: round(v, 4) for k, v in bx.worker_timing(i).items()} for i in range(bx.n_devices)]
    bx.close(); free_pinned(pin)
    mb = n_frames * w * h / 1e6
    return {"value": round(n_frames / best, 1), "unit": "frames/s", "frames": n_frames, "frames_in_flight": in_flight,
            "h2d_MBps": round(mb / best, 1), "worker_seconds": {k: round(v, 4) for k, v in tm.items()},
            "worker_numa_node": aff[0], "worker_cpus_bound": aff[1], "elapsed_max": elapsed_max,
            "per_worker_seconds": per_worker,   # (staging = host memory bandwidth: on 8 GPUs 8 x 13 GB/s of H2D are 105 GB/s of host reads -- the number to watch)
            "what": "plf_batch_extract: %d host frames (pinned, %d distinct) -> key points, descriptors, lines and local-map matches in host memory, 1 GPU" % (n_frames, nd)}


def cpu_baseline(seconds_target, threads, w, h, nfeat, nlines, family="polygons", single_only=False):
    """The CPU oracle (a port of the reference algorithm, kind="port") timed on this host, built HERE with the reference's flags
    (-O3 -march=native, /root/reference CMakeLists.txt:14): (a) one frame at a time on one thread, as Examples/RGB-D/rgbd_tum.cc:98-116 times
    it -- median / p95 and the per-stage split; (a2) ORB and LSD on two threads (PL-SLAM family); (b) one frame per thread on all cores."""
    import ctypes as C
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))   # tests/orc.py = the ctypes wrapper of the CPU oracle (the checker; only this leg uses it)
    import orc
    from rgbd_pl_slam_amd import matchgen
    from rgbd_pl_slam_amd.synth import synth_frame
    flags = "-O3 -march=native"
    try:
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "-s", "-B", "native"])
        L = C.CDLL(os.path.join(ROOT, "oracle", "liborc_native.so"))
    except Exception:
        L = orc.lib(); flags = "-O2 (the -O3 -march=native build failed on this host)"
    L.orc_frontend_throughput.restype = C.c_double
    L.orc_frontend_latency.restype = C.c_long
    frames = np.stack([_frame_fn(family)(5000 + i, w, h) for i in range(16)])
    r0 = orc.orb_extract(frames[0], nfeatures=nfeat)
    l0 = orc.line_extract(frames[0], nlines)
    mp = {k: np.ascontiguousarray(v) for k, v in matchgen.make_local_map(r0["kps"], r0["desc"], M_POINTS, 1, w=w, h=h).items()}
    ml = {k: np.ascontiguousarray(v) for k, v in matchgen.make_map_lines(l0["kl"], l0["desc"], M_LINES, 2).items()}
    MP = orc.MapPoints(); MP.m = M_POINTS
    for k in ("proj_x", "proj_y", "proj_xr", "level", "view_cos", "in_view", "desc", "obs_positive"):
        setattr(MP, k, orc.p(mp[k]).value)
    ML = orc.MapLines(); ML.m = M_LINES
    for k in ("x1", "y1", "x2", "y2", "level", "view_cos", "in_view", "desc"):
        setattr(ML, k, orc.p(ml[k]).value)
    common = (C.c_int(nfeat), C.c_int(nlines), C.byref(MP), C.byref(ML), C.c_float(3.0), C.c_float(0.8))

    def latency(n, warm, two):
        per = np.zeros(n, np.float64); st = np.zeros(16, np.float64)
        chk = L.orc_frontend_latency(orc.p(frames), C.c_int(16), C.c_int(w), C.c_int(h), C.c_int(n), C.c_int(warm), *common, C.c_int(two), orc.p(per), orc.p(st))
        return per, st, chk
    # (a) single thread: a probe frame sizes the sample to ~45 % of the budget
    per, _, _ = latency(2, 1, 0)
    n1 = int(max(10, min(200, 0.45 * seconds_target / max(float(np.median(per)), 1e-3))))
    per1, st1, chk1 = latency(n1, 3, 0)
    n2 = max(6, n1 // 4)
    per2, _, _ = latency(n2, 2, 1)
    names = ["pyramid", "fast", "octree", "orient", "blur", "brief", "lsd", "lbd", "match_points", "match_lines"]
    single = {"ms_median": round(1e3 * float(np.median(per1)), 2), "ms_p95": round(1e3 * float(np.percentile(per1, 95)), 2),
              "ms_mean": round(1e3 * float(per1.mean()), 2), "frames_per_s": round(1.0 / float(np.median(per1)), 2), "frames": n1, "warmup": 3,
              "stage_ms_per_frame": {nm: round(1e3 * float(st1[i]) / n1, 3) for i, nm in enumerate(names)},
              "orb_lsd_on_two_threads_ms_median": round(1e3 * float(np.median(per2)), 2), "two_thread_frames": n2}
    if single_only:      # (the real_photos block: the port on the same kind of frames, one at a time)
        single["kind"] = "port"; single["flags"] = flags; single["what"] = "the CPU port on 16 %dx%d frames of the family '%s', one at a time on one thread" % (w, h, family)
        return single

    def run(n, t):
        chk = C.c_long(0)
        return L.orc_frontend_throughput(orc.p(frames), C.c_int(16), C.c_int(w), C.c_int(h), C.c_int(n), C.c_int(t), *common, C.byref(chk))
    # (b) the visible CPU count can exceed what the container may really use: pick the thread count with the best measured throughput on a
    # short probe, then size the sample to the rest of the budget
    best_t, best_v = threads, 0.0
    for t in sorted({threads, max(1, threads // 2), min(threads, 64), min(threads, 32)}):
        d = run(2 * t, t)
        if 2 * t / d > best_v:
            best_v, best_t = 2 * t / d, t
    threads = best_t
    n = max(2 * threads, int(best_v * 0.35 * seconds_target))
    dt = run(n, threads)
    return {"value": round(n / dt, 2), "unit": "frames/s", "cores": threads, "kind": "port", "flags": flags,
            "sample": "%d synthetic %dx%d frames (16 distinct), same workload incl. map matching, one frame per OpenMP thread on %d threads, %.1f s; "
                      "single-thread figures: %d frames one at a time" % (n, w, h, threads, dt, n1),
            "per_core": round(n / dt / threads, 3), "single_thread": single}


def run_headline(args, dist, rank, local_rank, world, B, W, H, NFEAT, NLINES, label, make_pipe, timed_fn=None, reduce_device="cuda"):
    """The headline step on this rank and, on rank 0, the JSON line without the N = 1 extras.  The job is world * B frames per step; this rank's block of it comes
    from the product's partition (plf_batch_shard, contiguous blocks) and is always B frames: weak scaling.  make_pipe(nb) builds the device-resident pipeline
    (tests/test_sharding.py passes a stub and runs the rank logic -- partition, barrier, MAX over the ranks, assembly -- with world 8 on gloo).
    Returns (out or None, pipe, fps, elapsed, B)."""
    import torch
    from rgbd_pl_slam_amd.batch import shard
    timed_fn = timed_fn or timed
    lo, hi = shard(world * B, world, rank)
    assert hi - lo == B and lo == rank * B
    try:
        pipe = make_pipe(B)
    except Exception as e:   # (8192 frames in flight hold ~150 GB of the 288 GB: a GPU that cannot give them runs the 4096-frame workload, and says so)
        if args.batch > 0 or B <= 4096 or world > 1:
            raise
        sys.stderr.write("bench.py: %d frames in flight could not be set up (%r); falling back to 4096\n" % (B, e))
        torch.cuda.empty_cache()
        B = 4096
        pipe = make_pipe(B)
    elapsed, reg_ms, reg_launches = timed_fn(pipe, args.steps, args.warmup, dist)
    elapsed = reduce_elapsed_max(dist, elapsed, device=reduce_device)
    frames = world * B * args.steps
    fps = frames / elapsed
    if rank != 0:
        return None, pipe, fps, elapsed, B
    b_orb, b_line, b_region = algorithmic_bytes(W, H, NFEAT, NLINES)
    reg_avg_s = (reg_ms / max(reg_launches, 1)) * 1e-3
    # HBM traffic of the dominant kernel: PMC counters cannot be read from inside this process; they are collected with rocprofv3 --pmc in
    # separate passes on this very command (tools/pmc_traffic.py) and committed; scaled here to this run's batch
    traffic, traffic_source = None, None
    try:
        src = next((c for c in (os.path.join("profiles", "r%02d_pmc_traffic.json" % r) for r in (6, 5, 4, 3)) if os.path.exists(os.path.join(ROOT, c))), None)
        with open(os.path.join(ROOT, src)) as fh:
            pmc = json.load(fh)
        if (pmc.get("width"), pmc.get("height")) in ((W, H), (None, None)):
            traffic = int(pmc["region_kernel"]["hbm_bytes_per_launch"] * B / pmc["frames_per_launch"])
            traffic_source = "%s (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE of this command at %d frames per launch, scaled to %d)" % (src, pmc["frames_per_launch"], B)
    except Exception:
        traffic = None
    achieved = (b_region * B) / reg_avg_s / 1e9 if reg_avg_s > 0 else 0.0
    # share of the step during which an average SIMD's vector issue port is taken: counted VALU instructions per kernel (rocprofv3 --pmc SQ_INSTS_VALU of this
    # command, committed) x the issue interval of their class (2.2 / 4.2 / 8 / 16 cycles per SIMD, measured by tools/valu_issue.hip; mix per kernel from its ISA:
    # tools/classify_isa.py) over 1024 SIMDs x clock x the step time measured here
    valu_frac, valu_source = None, None
    try:
        vsrc = next(c for c in (os.path.join("profiles", "r%02d_valu_classes.json" % r) for r in (6, 5, 4)) if os.path.exists(os.path.join(ROOT, c)))
        with open(os.path.join(ROOT, vsrc)) as fh:
            vc = json.load(fh)
        if args.config == 2:
            cyc = vc["valu_issue_simd_cycles_per_step"] * B / vc["frames_per_step"]
            step_s = elapsed / args.steps
            valu_frac = round(cyc / (vc["simds"] * vc["clock_hz"] * step_s), 3)
            valu_source = ("%s: %.3g VALU wave-instructions per %d-frame step (SQ_INSTS_VALU), mean %.2f issue cycles each by class "
                           "(tools/classify_isa.py; intervals from profiles/r03_valu_issue.json)" % (vsrc, vc["valu_wave_instructions_per_step"], vc["frames_per_step"],
                                                                                                    vc["mean_cycles_per_valu"]))
    except Exception:
        valu_frac = None
    out = {
        "metric": "RGB-D frames/sec (ORB+LSD extract + BF-Hamming match) at %dx%d" % (W, H),
        "value": round(fps, 2), "unit": "frames/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": round(1e3 * elapsed / args.steps, 3), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "u8/f64", "data": "synthetic (%d independently seeded %dx%d frames per GPU tiled to the batch, resident in HBM; per-frame poses change every step)" % (pipe.ndist, W, H),
        "config": {"workload": label + "; matching per frame: SearchByProjection vs a %d-point local map + vs the last frame, line projection search vs %d map "
                                       "lines + brute-force Hamming kNN (k = 2) of the LBD descriptors vs the last frame's lines" % (M_POINTS, M_LINES),
                   "baseline_config": args.config, "frames_in_flight_per_gpu": B, "parallelism": "frames sharded over %d GPU(s) by contiguous blocks, no collective" % world},
        "matches_frame0": pipe.matches_frame0(),
        "pipeline_algorithmic_GBps": round(fps * (b_orb + b_line) / 1e9, 2),
        "roofline": {"bound": "hbm", "kernel": "LSD region growing (k_lsd_regions2 / k_lsd_spec_* for few frames in flight)", "achieved": round(achieved, 3),
                     "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBS, 6), "traffic": traffic, "traffic_source": traffic_source,
                     "avg_launch_ms": round(reg_avg_s * 1e3, 3), "launches": reg_launches, "algorithmic_bytes_per_launch": b_region * B,
                     "valu_issue_frac": valu_frac, "valu_issue_source": valu_source},
    }
    out["frames_of_this_rank"] = [lo, hi]
    # the whole path against the HBM roofline (algorithmic bytes per frame x frames/s / 8 TB/s), and the ten heaviest kernels one by one: algorithmic bytes
    # per launch (SURVEY 8d term), solo and overlapped duration (rocprofv3 --kernel-trace --stats of this command with --serial / as it is), counter traffic
    # (--pmc FETCH_SIZE + WRITE_SIZE) -- collected by tools/per_kernel_roofline.py in separate passes of this command and committed
    out["roofline"]["pipeline_frac"] = round(fps * (b_orb + b_line) / 1e9 / HBM_PEAK_GBS, 5)
    try:
        ksrc = next(c for c in (os.path.join("profiles", "r%02d_per_kernel.json" % r) for r in (6,)) if os.path.exists(os.path.join(ROOT, c)))
        with open(os.path.join(ROOT, ksrc)) as fh:
            pk = json.load(fh)
        if args.config == 2 and (pk.get("width"), pk.get("height")) == (W, H):
            out["roofline"]["per_kernel"] = pk["kernels"]
            out["roofline"]["per_kernel_source"] = "%s (%d frames per launch)" % (ksrc, pk["frames_per_launch"])
    except Exception:
        pass
    # vector-issue occupancy from COUNTERS: sum over the step's kernels of SQ_ACTIVE_INST_VALU (units of 4 cycles, one SIMD each) x 4 over
    # 1024 SIMDs x the cycles of the step measured here; beside the modelled valu_issue_frac
    try:
        isrc = next(c for c in (os.path.join("profiles", "r%02d_issue_counters.json" % r) for r in (6,)) if os.path.exists(os.path.join(ROOT, c)))
        with open(os.path.join(ROOT, isrc)) as fh:
            ic = json.load(fh)
        if args.config == 2:
            quads = ic["active_inst_valu_per_step"] * B / ic["frames_per_step"]
            out["roofline"]["valu_busy_frac"] = round(quads * 4.0 / (ic["simds"] * ic["clock_hz"] * (elapsed / args.steps)), 3)
            out["roofline"]["valu_busy_source"] = "%s: sum of SQ_ACTIVE_INST_VALU over the kernels of one %d-frame step" % (isrc, ic["frames_per_step"])
    except Exception:
        pass
    return out, pipe, fps, elapsed, B


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--config", type=int, default=2, choices=sorted(CONFIGS), help="BASELINE.json configs[] entry, counted from 1 (2 = the headline metric)")
    ap.add_argument("--batch", type=int, default=0, help="frames in flight per GPU and step (0: the config's own value)")
    ap.add_argument("--distinct", type=int, default=1024, help="independently seeded frames per GPU, tiled to the batch (the extra key tiled32 repeats the run with 32)")
    ap.add_argument("--full", action="store_true", help="also measure the secondary figures after the headline (tiled32, fps_vs_in_flight, config 3 as specified, "
                    "latency, PCIe-inclusive rate, natural and real-photograph frames, CPU baseline); off: the headline alone")
    ap.add_argument("--cpu-seconds", type=float, default=24.0, help="with --full: target duration of the CPU baseline sample (0: skip)")
    ap.add_argument("--no-extras", action="store_true", help="with --full: skip the secondary figures on the GPU (config 3 as specified, latency, PCIe-inclusive rate)")
    ap.add_argument("--line-handles", type=int, default=1, help="line extractor handles used alternately (1 or 2)")
    ap.add_argument("--no-front-wait", action="store_true", help="diagnostic: let ORB start together with the line front stages")
    ap.add_argument("--no-defer-match", action="store_true", help="diagnostic: enqueue the matchers of step k in step k (default: behind the line front stages of "
                    "step k+1, so that they run in the shadow of the next region-growing kernel; +2.7 %%)")
    ap.add_argument("--family", default="polygons", choices=["polygons", "natural", "photo"], help="diagnostic: image family of the main step (the headline is quoted on the "
                    "polygon scenes of SURVEY 8d; the `natural` extras run the natural-image-like family in the same run)")
    ap.add_argument("--serial", action="store_true", help="diagnostic: everything on one stream (solo kernel durations under rocprofv3)")
    ap.add_argument("--pcie", action="store_true", help="time the PCIe-INCLUSIVE leg instead (plf_batch_extract: pinned host frames in, features + local-map matches "
                    "out in host memory) on every rank; value = aggregate frames/s, plus the aggregate host read rate")
    ap.add_argument("--dump-outputs", metavar="DIR", help="after the timed steps, write what the last one computed as DIR/<name>.npy (a fixed seeded sample of "
                    "the frames, at most 64 MB; rank 0's frames)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")
    if args.dump_outputs and args.pcie:
        ap.error("--dump-outputs covers the device-resident step, not --pcie")

    import torch
    rank = int(os.environ.get("RANK", "0")); local_rank = int(os.environ.get("LOCAL_RANK", "0")); world = int(os.environ.get("WORLD_SIZE", "1"))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: the front-end has no CPU path")
    torch.cuda.set_device(local_rank)
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local_rank))

    from rgbd_pl_slam_amd.batch import shard
    W, H, NFEAT, NLINES, B0, label = CONFIGS[args.config]
    B = args.batch if args.batch > 0 else B0
    if args.pcie:
        line = run_pcie(args, dist, rank, local_rank, world, B, W, H, NFEAT, NLINES, label)
        if rank == 0:
            print(json.dumps(line))
        if dist is not None:
            dist.destroy_process_group()
        return
    def make_pipe(nb):
        return Pipeline(W, H, NFEAT, NLINES, nb, local_rank, 10_000 * rank, serial=args.serial, line_handles=args.line_handles, front_wait=not args.no_front_wait,
                        defer_match=not args.no_defer_match, distinct=args.distinct, family=args.family)
    out, pipe, fps, elapsed, B = run_headline(args, dist, rank, local_rank, world, B, W, H, NFEAT, NLINES, label, make_pipe)

    if rank == 0:
        if args.dump_outputs:
            out["dump_outputs"] = dump_outputs(pipe, args.dump_outputs)
        if world > 1 and args.full:
            out["extras"] = "skipped: tiled32 / fps_vs_in_flight / config3_as_specified / single_frame_latency / natural / pcie_inclusive / cpu_baseline are N = 1 figures"
        # (--full: the secondary figures below, each in runs of its own after the headline; a plain run skips them all)
        extras = args.full and world == 1 and args.config == 2 and not args.no_extras and not args.serial
        out["region_chain_length"] = pipe.chain_stats()
        out["nfa_rectangles_per_frame"] = pipe.rect_stats()
        if extras and pipe.ndist > 32:
            # the round-2 workload (32 distinct frames tiled to the batch), same pipeline object, same run: how much input diversity costs
            pipe.load_images(32)
            e32, r32, n32 = timed(pipe, args.steps, 1)
            out["tiled32"] = {"value": round(B * args.steps / e32, 2), "unit": "frames/s", "ms_per_step": round(1e3 * e32 / args.steps, 3),
                              "region_kernel_ms": round(r32 / max(n32, 1), 3), "region_chain_length": pipe.chain_stats(),
                              "what": "the same step on 32 distinct frames tiled to the batch (the round-1/2 workload)"}
        mp, ml = pipe.mp, pipe.ml
        pipe.close(); del pipe
        if extras:
            # where the 5,000 frames/s of BASELINE.json's target is crossed: the same step with fewer frames in flight (the few-frames schedules of the line
            # extractor take over below ~640)
            curve = []
            for nb in (8, 64, 512, 4096):
                if nb >= B:
                    continue
                pn = Pipeline(W, H, NFEAT, NLINES, nb, local_rank, 30_000, distinct=min(nb, 1024))
                k = 30 if nb <= 64 else (12 if nb <= 512 else 6)
                en, _, _ = timed(pn, k, 3)
                curve.append({"frames_in_flight": nb, "value": round(nb * k / en, 1), "ms_per_step": round(1e3 * en / k, 3)})
                pn.close(); del pn
            curve.append({"frames_in_flight": B, "value": round(fps, 1), "ms_per_step": round(1e3 * elapsed / args.steps, 3)})
            out["fps_vs_in_flight"] = {"unit": "frames/s", "points": curve, "what": "the default step (config 2 workload) at fewer frames in flight, same run"}
        if extras:
            # secondary figures, driver-timed in the same run
            p3 = Pipeline(*CONFIGS[3][:5], local_rank, 20_000)
            e3, r3, n3 = timed(p3, 30, 5)
            out["config3_as_specified"] = {"value": round(8 * 30 / e3, 1), "unit": "frames/s", "ms_per_step": round(1e3 * e3 / 30, 3), "what": CONFIGS[3][5],
                                           "region_stage_ms": round(r3 / max(n3, 1), 3)}
            p3.close(); del p3
            out["single_frame_latency"] = single_frame_latency(local_rank, W, H, NFEAT, NLINES)
            # the reference's own operating regime: one frame per TrackRGBD call, extraction AND the tracking matchers (round 5: the matchers of a single frame had
            # never been timed -- the last-frame search alone took 2.7 ms per 1000 key points)
            out["tracking_call_latency"] = {"config2": tracking_call_latency(local_rank, 2), "config3_one_frame": tracking_call_latency(local_rank, 3),
                                            "config2_natural": tracking_call_latency(local_rank, 2, family="natural")}
            out["pcie_inclusive"] = pcie_inclusive(local_rank, W, H, NFEAT, NLINES, 16384, 4096, mp, ml)
            out["pcie_inclusive"].pop("elapsed_max", None)
        if extras:
            # natural-image-like frames (synth.natural_frame) through the same step: large batch, 8 in flight, one frame
            nat = {"what": "the default step on natural-image-like frames (1/f texture + lens-blurred scene + shot / read noise: synth.natural_frame) instead of "
                           "the hard-edged polygon scenes; same workload, same run"}
            pn = Pipeline(W, H, NFEAT, NLINES, B, local_rank, 40_000, distinct=args.distinct, family="natural")
            en, rn, nn = timed(pn, args.steps, args.warmup)
            nat["in_flight_%d" % B] = {"value": round(B * args.steps / en, 2), "unit": "frames/s", "ms_per_step": round(1e3 * en / args.steps, 3),
                                       "region_kernel_ms": round(rn / max(nn, 1), 3), "region_chain_length": pn.chain_stats(), "nfa_rectangles_per_frame": pn.rect_stats(),
                                       "lines_kept_mean": pn.lines_kept(), "vs_polygons": round((B * args.steps / en) / fps, 3)}
            pn.close(); del pn
            pn = Pipeline(W, H, NFEAT, NLINES, 8, local_rank, 41_000, distinct=8, family="natural")
            en, rn, nn = timed(pn, 30, 5)
            nat["in_flight_8"] = {"value": round(8 * 30 / en, 1), "unit": "frames/s", "ms_per_step": round(1e3 * en / 30, 3), "region_stage_ms": round(rn / max(nn, 1), 3),
                                  "validation_rounds": pn.rounds_stats(), "nfa_rectangles_per_frame": pn.rect_stats(), "lines_kept_mean": pn.lines_kept()}
            pn.close(); del pn
            nat["single_frame"] = single_frame_latency(local_rank, W, H, NFEAT, NLINES, family="natural")
            out["natural"] = nat
            # REAL photographs (tests/golden/real: seven CC0 / public-domain photographs; synth.photo_frame cuts VGA windows out of them at their native scale and
            # extends them by reflection): no TUM frame exists here or on the GPU box, these are the real-camera input the image offers
            rp = {"what": "the default step on windows of real photographs (tests/golden/real, CC0 / public domain: camera man, astronaut, coffee cup, cat, bricks, "
                          "grass, gravel) instead of synthetic frames; same workload, same run"}
            pn = Pipeline(W, H, NFEAT, NLINES, B, local_rank, 50_000, distinct=args.distinct, family="photo")
            en, rn, nn = timed(pn, args.steps, args.warmup)
            rp["in_flight_%d" % B] = {"value": round(B * args.steps / en, 2), "unit": "frames/s", "ms_per_step": round(1e3 * en / args.steps, 3),
                                      "region_kernel_ms": round(rn / max(nn, 1), 3), "region_chain_length": pn.chain_stats(), "nfa_rectangles_per_frame": pn.rect_stats(),
                                      "lines_kept_mean": pn.lines_kept(), "vs_polygons": round((B * args.steps / en) / fps, 3)}
            pn.close(); del pn
            pn = Pipeline(W, H, NFEAT, NLINES, 8, local_rank, 51_000, distinct=8, family="photo")
            en, rn, nn = timed(pn, 30, 5)
            rp["in_flight_8"] = {"value": round(8 * 30 / en, 1), "unit": "frames/s", "ms_per_step": round(1e3 * en / 30, 3), "region_stage_ms": round(rn / max(nn, 1), 3),
                                 "lines_kept_mean": pn.lines_kept()}
            pn.close(); del pn
            rp["single_frame"] = single_frame_latency(local_rank, W, H, NFEAT, NLINES, family="photo")
            rp["tracking_call"] = tracking_call_latency(local_rank, 2, family="photo")
            if args.cpu_seconds > 0:
                rp["cpu_port_single_thread"] = cpu_baseline(min(8.0, float(args.cpu_seconds)), 1, W, H, NFEAT, NLINES, family="photo", single_only=True)
            out["real_photos"] = rp
        if args.full and world == 1 and args.cpu_seconds > 0:
            cores = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
            out["cpu_baseline"] = cpu_baseline(float(args.cpu_seconds), cores, W, H, NFEAT, NLINES)
        print(json.dumps(out))
    else:
        pipe.close()
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
