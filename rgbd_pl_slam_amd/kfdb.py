"""ORB_SLAM2::KeyFrameDatabase on the GPU: add / erase / clear, DetectRelocalizationCandidates and DetectLoopCandidates.
A thin mirror of the plf_kfdb_* entry points of include/plf.h; the compute is HIP (csrc/kfdb_kernels.hip).  Keyframes are slots
0 .. max_keyframes - 1; BoW vectors come as the dict `Vocabulary.transform` returns and never leave the device."""
import ctypes as C

import numpy as np

from . import _lib as L


class KeyFrameDatabase:
    def __init__(self, vocabulary, max_keyframes, capacity):
        self._lib = L.kfdb_prototypes(L.lib())
        self._h = None
        h = C.c_void_p()
        L.check(self._lib.plf_kfdb_create(getattr(vocabulary, "_h", None), int(max_keyframes), int(capacity), C.byref(h)), "plf_kfdb_create")
        self._h = h
        self._voc = vocabulary                   # the handle holds no reference of its own: keep the vocabulary alive
        self.max_keyframes, self.capacity = int(max_keyframes), int(capacity)

    def close(self):
        if self._h:
            self._lib.plf_kfdb_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self):
        """live keyframes, entries of the inverted file (rebuilds a stale one and waits)"""
        i = L.KfdbInfo()
        L.check(self._lib.plf_kfdb_info(self._h, C.byref(i)), "plf_kfdb_info")
        return {name: getattr(i, name) for name, _ in L.KfdbInfo._fields_}

    def set_n_best(self, n_best):
        L.check(self._lib.plf_kfdb_set_n_best(self._h, int(n_best)), "plf_kfdb_set_n_best")

    @staticmethod
    def _bow(bow):
        import torch
        wid, val, n = bow["word_id"], bow["word_val"], bow["n_words"]
        if wid.dim() == 1:
            wid, val = wid[None], val[None]
        assert wid.is_cuda and val.is_cuda and n.is_cuda and wid.dtype == torch.int32 and val.dtype == torch.float64 and n.dtype == torch.int32
        assert wid.is_contiguous() and val.is_contiguous() and wid.shape == val.shape and n.numel() == wid.shape[0]
        return wid, val, n, int(wid.shape[0]), int(wid.shape[1])

    @staticmethod
    def _stream(stream):
        return C.c_void_p(stream) if stream else None

    def add(self, bow, slots, stream=None):
        """KeyFrameDatabase::add for the frames of `bow` (the dict Vocabulary.transform returns), in index order; frame f goes to slots[f]"""
        wid, val, n, F, cap = self._bow(bow)
        slots = np.ascontiguousarray(slots, np.int32).reshape(-1)
        assert len(slots) == F
        L.check(self._lib.plf_kfdb_add_batch(self._h, L.vp(wid), L.vp(val), L.vp(n), F, cap, L.vp(slots), self._stream(stream)), "plf_kfdb_add_batch")

    def erase(self, slots):
        slots = np.ascontiguousarray(slots, np.int32).reshape(-1)
        L.check(self._lib.plf_kfdb_erase_batch(self._h, L.vp(slots), len(slots)), "plf_kfdb_erase_batch")

    def clear(self):
        L.check(self._lib.plf_kfdb_clear(self._h), "plf_kfdb_clear")

    def vectors(self):
        """device addresses of the resident vectors: (word_id, word_val, n_words), slot s at s * capacity"""
        a, b, c = C.c_void_p(), C.c_void_p(), C.c_void_p()
        L.check(self._lib.plf_kfdb_vectors(self._h, C.byref(a), C.byref(b), C.byref(c)), "plf_kfdb_vectors")
        return a.value, b.value, c.value

    def _out(self, Q, max_cand, dev):
        """uninitialised on purpose: a torch fill would run on torch's stream, unordered with the stream the call writes them on; the call
        itself sets every entry (cand to -1 beyond the count)"""
        import torch
        return (torch.empty((Q, max_cand), dtype=torch.int32, device=dev), torch.empty(Q, dtype=torch.int32, device=dev),
                torch.empty((Q, 4), dtype=torch.int32, device=dev))

    @staticmethod
    def _csr(csr):
        import torch
        if csr is None:
            return None, None
        start, idx = csr
        assert start.is_cuda and idx.is_cuda and start.dtype == torch.int32 and idx.dtype == torch.int32
        return start, idx

    def detect_relocalization_candidates(self, bow, covis=None, max_cand=64, stream=None):
        """DetectRelocalizationCandidates for every frame of `bow`, as if called one by one in index order.  covis = (start, slot): int32
        device tensors, the CSR of every slot's ordered covisible keyframes.  Returns device tensors cand (Q, max_cand) int32 (-1 beyond
        the count), n_cand (Q,), stats (Q, 4) int32 (view the last column as float32: bestAccScore; _lib.KFDB_STATS_DTYPE).  Only enqueues."""
        wid, val, n, Q, cap = self._bow(bow)
        cs, ci = self._csr(covis)
        cand, n_cand, stats = self._out(Q, max_cand, wid.device)
        L.check(self._lib.plf_kfdb_detect_reloc(self._h, L.vp(wid), L.vp(val), L.vp(n), Q, cap, L.vp(cs), L.vp(ci), max_cand, L.vp(cand), L.vp(n_cand),
                                                L.vp(stats), self._stream(stream)), "plf_kfdb_detect_reloc")
        return cand, n_cand, stats

    def detect_loop_candidates(self, bow, min_score, covis=None, connected=None, max_cand=64, stream=None):
        """DetectLoopCandidates.  min_score: (Q,) float32 device tensor; connected = (start, slot): the CSR over the queries of each query's
        GetConnectedKeyFrames() (and the query's own slot, if it is already in the database)."""
        import torch
        wid, val, n, Q, cap = self._bow(bow)
        cs, ci = self._csr(covis)
        es, ei = self._csr(connected)
        assert min_score.is_cuda and min_score.dtype == torch.float32 and min_score.numel() == Q
        cand, n_cand, stats = self._out(Q, max_cand, wid.device)
        L.check(self._lib.plf_kfdb_detect_loop(self._h, L.vp(wid), L.vp(val), L.vp(n), Q, cap, L.vp(cs), L.vp(ci), L.vp(es), L.vp(ei), L.vp(min_score),
                                               max_cand, L.vp(cand), L.vp(n_cand), L.vp(stats), self._stream(stream)), "plf_kfdb_detect_loop")
        return cand, n_cand, stats

    DetectRelocalizationCandidates = detect_relocalization_candidates
    DetectLoopCandidates = detect_loop_candidates
