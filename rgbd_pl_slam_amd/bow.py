"""DBoW2 vocabulary on the GPU: ORBVocabulary::transform (Frame::ComputeBoW / KeyFrame::ComputeBoW) and ORBVocabulary::score.
A thin mirror of the plf_vocab_* / plf_bow_* entry points of include/plf.h; the compute is HIP (csrc/bow_kernels.hip)."""
import ctypes as C

import numpy as np

from . import _lib as L


def parse_text(path):
    """plf_vocab_parse_text: the vocabulary text file as numpy arrays (host only, no GPU needed)"""
    lib = L.bow_prototypes(L.lib())
    d = L.VocabDesc()
    L.check(lib.plf_vocab_parse_text(str(path).encode(), C.byref(d)), "plf_vocab_parse_text")
    try:
        n = d.n_nodes
        arr = lambda p, ct, cnt, dt: np.frombuffer(C.string_at(p, C.sizeof(ct) * cnt), dt).copy()
        return {"k": d.k, "L": d.L, "scoring": d.scoring, "weighting": d.weighting,
                "parent": arr(d.parent, C.c_int32, n, np.int32), "desc": arr(d.desc, C.c_uint8, n * 32, np.uint8).reshape(n, 32),
                "weight": arr(d.weight, C.c_double, n, np.float64), "is_leaf": arr(d.is_leaf, C.c_uint8, n, np.uint8)}
    finally:
        lib.plf_vocab_desc_free(C.byref(d))


class Vocabulary:
    """ORB_SLAM2::ORBVocabulary.  `transform` returns device tensors laid out as plf_bow_view / plf_tri_view read them."""

    def __init__(self, handle):
        self._lib = L.bow_prototypes(L.lib())
        self._h = handle
        info = L.VocabInfo()
        L.check(self._lib.plf_vocab_info(self._h, C.byref(info)), "plf_vocab_info")
        for name, _ in L.VocabInfo._fields_:
            setattr(self, name, getattr(info, name))

    @classmethod
    def from_text(cls, path, device=0):
        lib = L.bow_prototypes(L.lib())
        h = C.c_void_p()
        L.check(lib.plf_vocab_load_text(str(path).encode(), device, C.byref(h)), "plf_vocab_load_text")
        return cls(h)

    @classmethod
    def from_arrays(cls, k, Lv, scoring, weighting, parent, desc, weight, is_leaf, device=0):
        lib = L.bow_prototypes(L.lib())
        parent = np.ascontiguousarray(parent, np.int32); desc = np.ascontiguousarray(desc, np.uint8)
        weight = np.ascontiguousarray(weight, np.float64); is_leaf = np.ascontiguousarray(is_leaf, np.uint8)
        n = len(parent)
        assert desc.size == n * 32 and len(weight) == n and len(is_leaf) == n
        d = L.VocabDesc(k, Lv, scoring, weighting, n, parent.ctypes.data, desc.ctypes.data, weight.ctypes.data, is_leaf.ctypes.data)
        h = C.c_void_p()
        L.check(lib.plf_vocab_create(C.byref(d), device, C.byref(h)), "plf_vocab_create")
        return cls(h)

    def close(self):
        if self._h:
            self._lib.plf_vocab_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def transform(self, desc, n_desc, levelsup=4, stream=None):
        """desc: (n_frames, capacity, 32) uint8 device tensor (the extractor's output), n_desc: (n_frames,) int32 device tensor.
        Returns a dict of device tensors: word_id (F, cap) int32 holding the uint32 ids, word_val (F, cap) float64, n_words (F,),
        node_id (F, cap), node_start (F, cap + 1), feat (F, cap), n_nodes (F,).  Only enqueues: on `stream` (a raw HIP stream, e.g. torch.cuda.Stream().cuda_stream), or on
        the vocabulary's own stream when none is given -- as with the other mirrors, synchronise the device before reading the outputs then."""
        import torch
        assert desc.is_cuda and n_desc.is_cuda and desc.dtype == torch.uint8 and n_desc.dtype == torch.int32
        if desc.dim() == 2:
            desc = desc[None]
        F, cap = int(desc.shape[0]), int(desc.shape[1])
        assert desc.is_contiguous() and desc.shape[2] == 32 and n_desc.numel() == F
        dev = desc.device
        out = {"word_id": torch.empty((F, cap), dtype=torch.int32, device=dev), "word_val": torch.empty((F, cap), dtype=torch.float64, device=dev),
               "n_words": torch.empty(F, dtype=torch.int32, device=dev), "node_id": torch.empty((F, cap), dtype=torch.int32, device=dev),
               "node_start": torch.empty((F, cap + 1), dtype=torch.int32, device=dev), "feat": torch.empty((F, cap), dtype=torch.int32, device=dev),
               "n_nodes": torch.empty(F, dtype=torch.int32, device=dev)}
        L.check(self._lib.plf_bow_transform_batch(self._h, L.vp(desc), L.vp(n_desc), F, cap, levelsup, L.MEM_DEVICE, L.MEM_DEVICE, L.vp(out["word_id"]),
                                                  L.vp(out["word_val"]), L.vp(out["n_words"]), L.vp(out["node_id"]), L.vp(out["node_start"]),
                                                  L.vp(out["feat"]), L.vp(out["n_nodes"]), C.c_void_p(stream) if stream else None), "plf_bow_transform_batch")
        return out

    def transform_host(self, desc, n_desc, levelsup=4):
        """the same call with host (numpy) memory on both sides; synchronises"""
        desc = np.ascontiguousarray(desc, np.uint8)
        if desc.ndim == 2:
            desc = desc[None]
        F, cap = desc.shape[0], desc.shape[1]
        n_desc = np.ascontiguousarray(n_desc, np.int32).reshape(F)
        out = {"word_id": np.zeros((F, cap), np.uint32), "word_val": np.zeros((F, cap), np.float64), "n_words": np.zeros(F, np.int32),
               "node_id": np.zeros((F, cap), np.uint32), "node_start": np.zeros((F, cap + 1), np.int32), "feat": np.zeros((F, cap), np.int32),
               "n_nodes": np.zeros(F, np.int32)}
        L.check(self._lib.plf_bow_transform_batch(self._h, L.vp(desc), L.vp(n_desc), F, cap, levelsup, L.MEM_HOST, L.MEM_HOST, L.vp(out["word_id"]),
                                                  L.vp(out["word_val"]), L.vp(out["n_words"]), L.vp(out["node_id"]), L.vp(out["node_start"]),
                                                  L.vp(out["feat"]), L.vp(out["n_nodes"]), None), "plf_bow_transform_batch")
        return out

    def score(self, q_word_id, q_val, db_word_id, db_val, db_start):
        """ORBVocabulary::score of one query vector against the M vectors of a CSR (db_start: M + 1).  numpy in, numpy (M,) float64 out."""
        q_id = np.ascontiguousarray(q_word_id).astype(np.uint32, copy=False); qv = np.ascontiguousarray(q_val, np.float64)
        d_id = np.ascontiguousarray(db_word_id).astype(np.uint32, copy=False); dv = np.ascontiguousarray(db_val, np.float64)
        st = np.ascontiguousarray(db_start, np.int32)
        M = len(st) - 1
        out = np.zeros(M, np.float64)
        L.check(self._lib.plf_bow_score(self._h, L.vp(q_id), L.vp(qv), len(q_id), L.vp(d_id), L.vp(dv), L.vp(st), M, L.vp(out), L.MEM_HOST, None),
                "plf_bow_score")
        return out
