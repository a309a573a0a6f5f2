"""DBoW2 vocabulary transform (Frame::ComputeBoW / KeyFrame::ComputeBoW) and BoW scores on the GPU against the numpy restatement tests/bowref.py.
Every comparison is bit for bit: word values and scores through .view(np.uint64), no tolerance."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import bowref
import orc
from conftest import gpu_available
from cppbuild import build_driver

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
WEIGHTINGS = (bowref.TF_IDF, bowref.TF, bowref.IDF, bowref.BINARY)
SCORINGS = (bowref.L1_NORM, bowref.L2_NORM, bowref.DOT_PRODUCT, bowref.CHI_SQUARE)   # CHI_SQUARE: an L1-normalised type whose score is out of scope


@pytest.fixture(autouse=True)
def _need_gpu():
    if not gpu_available():
        pytest.fail("no GPU visible: the -m gpu tests need a real MI355X")


def _vocab(ref):
    from rgbd_pl_slam_amd import Vocabulary
    V = Vocabulary.from_arrays(ref.k, ref.L, ref.scoring, ref.weighting, ref.parent, ref.desc, ref.weight, ref.is_leaf)
    assert (V.n_nodes, V.n_words, V.min_leaf_depth, V.k, V.L) == (ref.n_nodes(), ref.n_words, ref.min_leaf_depth, ref.k, ref.L)
    return V


def _pack(frames, cap):
    """list of (n_f, 32) arrays -> (F, cap, 32) with 0xA5 filler beyond n_f (must not be read), n_desc"""
    d = np.full((len(frames), cap, 32), 0xA5, np.uint8)
    for f, a in enumerate(frames):
        d[f, :len(a)] = a
    return d, np.array([len(a) for a in frames], np.int32)


def _host(out):
    """device outputs on the host.  A transform without a stream runs on the vocabulary's own stream, which torch's streams do not order with:
    wait for the device first."""
    import torch
    torch.cuda.synchronize()
    h = {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in out.items()}
    h["word_id"] = h["word_id"].view(np.uint32); h["node_id"] = h["node_id"].view(np.uint32)
    return h


def _assert_frame(h, f, ref_bow, ref_fv, what=""):
    cap = h["word_id"].shape[1]
    r = bowref.flatten(ref_bow, ref_fv, cap)
    nw, nn = int(h["n_words"][f]), int(h["n_nodes"][f])
    assert nw == r["n_words"] and nn == r["n_nodes"], (what, f, nw, r["n_words"], nn, r["n_nodes"])
    assert np.array_equal(h["word_id"][f, :nw], r["word_id"][:nw]), (what, f)
    assert np.array_equal(h["word_val"][f, :nw].view(np.uint64), r["word_val"][:nw].view(np.uint64)), (what, f)
    assert np.array_equal(h["node_id"][f, :nn], r["node_id"][:nn]), (what, f)
    assert np.array_equal(h["node_start"][f, :nn + 1], r["node_start"][:nn + 1]), (what, f)
    m = int(r["node_start"][nn])
    assert np.array_equal(h["feat"][f, :m], r["feat"][:m]), (what, f)


def _check(ref, V, frames, cap, levelsup, what=""):
    import torch
    d, n = _pack(frames, cap)
    out = V.transform(torch.from_numpy(d).cuda(), torch.from_numpy(n).cuda(), levelsup)
    torch.cuda.synchronize()
    h = _host(out)
    for f, a in enumerate(frames):
        bow, fv = bowref.transform(ref, a, levelsup)
        _assert_frame(h, f, bow, fv, what)
    return h


def test_device_double_division_and_sqrt_are_correctly_rounded():
    """the transform's only non-trivial double operations, isolated and checked against numpy (IEEE, correctly rounded) rather than assumed: two-word frames
    give w1 / (w1 + w2) under L1 and w1 / sqrt(w1 * w1 + w2 * w2) under L2, over 4096 frames with leaf weights spanning 40 binades"""
    import torch
    rng = np.random.default_rng(3)
    n = 4096
    for scoring in (bowref.L1_NORM, bowref.L2_NORM):
        ref = bowref.make_vocab(8, 20, 2, bowref.IDF, scoring)
        leaves = np.flatnonzero(ref.is_leaf > 0)
        ref.weight[leaves] = np.exp(rng.uniform(-14, 14, len(leaves)))
        V = _vocab(ref)
        d = rng.integers(0, 256, (n, 2, 32), dtype=np.uint8)
        h = _host(V.transform(torch.from_numpy(d).cuda(), torch.full((n,), 2, dtype=torch.int32, device="cuda"), 2))
        torch.cuda.synchronize()
        word, wt, _ = bowref.descend(ref, d.reshape(-1, 32), 2)
        wt = wt.reshape(n, 2); word = word.reshape(n, 2)
        checked = 0
        for f in range(n):
            if word[f, 0] == word[f, 1]:
                continue
            o = np.argsort(word[f]); a, b = np.float64(wt[f, o[0]]), np.float64(wt[f, o[1]])
            s = np.float64(0.0) + a + b if scoring == bowref.L1_NORM else np.sqrt(np.float64(0.0) + a * a + b * b)
            exp = np.array([a / s, b / s])
            assert int(h["n_words"][f]) == 2 and np.array_equal(h["word_val"][f].view(np.uint64), exp.view(np.uint64)), (scoring, f)
            checked += 1
        assert checked > n * 0.9


def test_hand_worked_fixture():
    from rgbd_pl_slam_amd import Vocabulary
    import torch
    fx = json.load(open(os.path.join(GOLD, "bow_tiny.json")))
    V = Vocabulary.from_text(os.path.join(GOLD, "bow_tiny_voc.txt"))
    assert (V.k, V.L, V.scoring, V.weighting, V.n_nodes, V.n_words, V.min_leaf_depth) == (3, 2, 0, 0, 13, 9, 2)
    desc = np.array(fx["descriptors"], np.uint8)
    for lu, fv_exp in fx["fv"].items():
        h = _host(V.transform(torch.from_numpy(desc[None]).cuda(), torch.tensor([len(desc)], dtype=torch.int32, device="cuda"), int(lu)))
        _assert_frame(h, 0, [(w, v) for w, v in fx["bow"]], [(n, f) for n, f in fv_exp], "levelsup " + lu)
    assert h["word_val"][0, 0] == 0.6 / fx["l1_norm"] != (6 * 0.1) / fx["l1_norm"]


# full trees where they fit; k = 10 / 20 at L = 6 as trees whose inner nodes beyond the first `full` of a level have a single child (every leaf stays at depth L,
# so every levelsup is legal); the complete k = 10, L = 6 tree has a test of its own below
@pytest.mark.parametrize("k,Lv,full", [(2, 1, None), (2, 3, None), (2, 6, None), (10, 1, None), (10, 3, None), (10, 6, 40), (20, 1, None), (20, 3, None), (20, 6, 30)])
def test_weightings_scorings_levelsup(k, Lv, full):
    rng = np.random.default_rng(k * 100 + Lv)
    for weighting in WEIGHTINGS:
        for scoring in SCORINGS:
            ref = bowref.make_vocab(1000 + k * 10 + Lv, k, Lv, weighting, scoring, zero_share=0.1, dup_share=0.15, full=full)
            assert ref.min_leaf_depth == Lv
            V = _vocab(ref)
            frames = [bowref.make_descriptors(ref, int(rng.integers(1 << 30)), n) for n in (257, 40)]
            frames.append(rng.integers(0, 256, (100, 32), dtype=np.uint8))
            for levelsup in sorted({0, 2, 4, Lv, Lv + 1}):
                _check(ref, V, frames, 300, levelsup, "k%d L%d w%d s%d lu%d" % (k, Lv, weighting, scoring, levelsup))
            V.close()


def test_edge_cases_ties_zero_weights_empty_identical_and_capacity_limit():
    from rgbd_pl_slam_amd import _lib as L
    rng = np.random.default_rng(9)
    ref = bowref.make_vocab(77, 10, 3, bowref.TF_IDF, bowref.L1_NORM, zero_share=0.3, dup_share=0.5, uneven=True, shallow_share=0.0)
    V = _vocab(ref)
    one = bowref.make_descriptors(ref, 1, 1)
    same = np.repeat(bowref.make_descriptors(ref, 2, 1), 500, axis=0)            # all identical: one word hit 500 times, sequential adds
    leaves = np.flatnonzero((ref.is_leaf > 0) & (ref.weight > 0))
    exact = ref.desc[leaves[rng.integers(0, len(leaves), 300)]]                  # copies of node descriptors: distance-0 ties among duplicated siblings
    zero_only = ref.desc[np.flatnonzero((ref.is_leaf > 0) & (ref.weight == 0))[:20]]
    frames = [np.zeros((0, 32), np.uint8), one, same, exact, zero_only, bowref.make_descriptors(ref, 3, 777)]
    for levelsup in (0, 1, 3, 5):
        h = _check(ref, V, frames, 800, levelsup)
        assert h["n_words"][0] == 0 and h["n_nodes"][0] == 0 and h["node_start"][0, 0] == 0 and h["n_words"][1] <= 1 and h["n_words"][2] <= 1
    # capacity at the stated limit: 8192 descriptors in one frame, beside a short one
    assert L.BOW_MAX_CAPACITY == 8192
    big = bowref.make_descriptors(ref, 4, 8192)
    _check(ref, V, [big, one, same], 8192, 2)
    import torch
    with pytest.raises(Exception) as e:
        V.transform(torch.zeros((1, 8193, 32), dtype=torch.uint8, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda"), 2)
    assert e.value.status == L.PLF_E_BADARG
    # 32 lanes per descriptor: a node with more than 16 children
    ref = bowref.make_vocab(78, 20, 2, bowref.TF, bowref.L2_NORM, dup_share=0.3)
    _check(ref, _vocab(ref), [bowref.make_descriptors(ref, 5, 1000, noise_bits=60)], 1000, 1)


def test_shallow_leaf_is_refused():
    from rgbd_pl_slam_amd import _lib as L
    import torch
    ref = bowref.make_vocab(5, 4, 4, bowref.TF_IDF, bowref.L1_NORM, shallow_share=0.3)
    assert ref.min_leaf_depth == 1
    V = _vocab(ref)
    d = torch.from_numpy(bowref.make_descriptors(ref, 1, 64)[None]).cuda(); n = torch.tensor([64], dtype=torch.int32, device="cuda")
    for levelsup in (0, 1, 2):          # L - levelsup = 4, 3, 2 > the shallowest leaf
        with pytest.raises(Exception) as e:
            V.transform(d, n, levelsup)
        assert e.value.status == L.PLF_E_BADARG
    for levelsup in (3, 4, 5):          # level 1 or the root: defined for every leaf
        _check(ref, V, [bowref.make_descriptors(ref, 1, 64)], 64, levelsup)


def test_full_size_tree_64_frames_of_2000():
    """k = 10, L = 6: 1.1 M nodes (35 MB of descriptors), generated on the fly"""
    ref = bowref.make_vocab(2024, 10, 6, bowref.TF_IDF, bowref.L1_NORM, zero_share=0.02)
    assert ref.n_nodes() == 1111111
    V = _vocab(ref)
    frames = [bowref.make_descriptors(ref, 100 + f, 2000 - 13 * f, noise_bits=30) for f in range(64)]
    _check(ref, V, frames, 2000, 4)


def test_host_memory_equals_device_memory():
    import torch
    ref = bowref.make_vocab(31, 10, 3, bowref.TF_IDF, bowref.L2_NORM, zero_share=0.1, dup_share=0.2)
    V = _vocab(ref)
    frames = [bowref.make_descriptors(ref, s, n) for s, n in ((1, 500), (2, 0), (3, 37))]
    d, n = _pack(frames, 512)
    dev = _host(V.transform(torch.from_numpy(d).cuda(), torch.from_numpy(n).cuda(), 2))
    torch.cuda.synchronize()
    host = V.transform_host(d, n, 2)
    for f, a in enumerate(frames):
        bow, fv = bowref.transform(ref, a, 2)
        _assert_frame(dev, f, bow, fv, "device"); _assert_frame(host, f, bow, fv, "host")


def test_scores():
    from rgbd_pl_slam_amd import _lib as L
    rng = np.random.default_rng(12)
    for scoring in (bowref.L1_NORM, bowref.L2_NORM, bowref.DOT_PRODUCT):
        ref = bowref.make_vocab(50 + scoring, 10, 3, bowref.TF_IDF, scoring, zero_share=0.05)
        V = _vocab(ref)
        sizes = [300, 0, 1, 1000, 70, 300] + [int(x) for x in rng.integers(1, 600, 40)]
        vecs = [bowref.transform(ref, bowref.make_descriptors(ref, 200 + j, n, noise_bits=10), 2)[0] for j, n in enumerate(sizes)]
        vecs.append(vecs[0])                                      # the query itself: L2 runs into its `score >= 1` clamp or next to it
        start = np.concatenate([[0], np.cumsum([len(v) for v in vecs])]).astype(np.int32)
        ids = np.array([w for v in vecs for w, _ in v], np.uint32); vals = np.array([x for v in vecs for _, x in v], np.float64)
        for q in (vecs[0], vecs[3], vecs[1], vecs[4]):            # longer, shorter and empty queries
            got = V.score(np.array([w for w, _ in q], np.uint32), np.array([x for _, x in q], np.float64), ids, vals, start)
            exp = np.array([bowref.score(scoring, q, v) for v in vecs], np.float64)
            assert np.array_equal(got.view(np.uint64), exp.view(np.uint64)), scoring
        assert np.count_nonzero(exp) > 20
    for scoring in (bowref.CHI_SQUARE, bowref.KL, bowref.BHATTACHARYYA):
        ref = bowref.make_vocab(60, 3, 2, bowref.TF_IDF, scoring)
        V = _vocab(ref)
        with pytest.raises(Exception) as e:
            V.score(ids[:3], vals[:3], ids[:3], vals[:3], np.array([0, 3], np.int32))
        assert e.value.status == L.PLF_E_BADARG


def test_extract_transform_search_by_bow_end_to_end():
    """ORBextractor (device output) -> Vocabulary.transform (device in, device out) -> plf_match_bow, against orc.search_by_bow fed with bowref's vectors"""
    import torch
    from rgbd_pl_slam_amd import ORBextractor, Matcher
    from rgbd_pl_slam_amd.synth import synth_frame
    w, h = 640, 480
    img = synth_frame(77, w, h)
    imgs = np.stack([img, np.roll(img, (3, 5), axis=(0, 1))])
    ext = ORBextractor(nfeatures=1000, max_width=w, max_height=h, max_batch=2)
    cap = ext.capacity
    kps = torch.zeros((2, cap, 7), dtype=torch.float32, device="cuda"); desc = torch.zeros((2, cap, 32), dtype=torch.uint8, device="cuda")
    n = torch.zeros(2, dtype=torch.int32, device="cuda")
    d_imgs = torch.from_numpy(imgs).cuda()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()                                        # one stream orders the three stages; nothing waits on the host in between
    ext.extract_batch_device(d_imgs, w, h, kps, desc, n, cap, s.cuda_stream)
    ref = bowref.make_vocab(4242, 10, 4, bowref.TF_IDF, bowref.L1_NORM, zero_share=0.01)
    V = _vocab(ref)
    out = V.transform(desc, n, 2, stream=s.cuda_stream)            # the extractor's device output, as it is
    torch.cuda.synchronize()
    nh = n.cpu().numpy(); hd = desc.cpu().numpy(); hh = _host(out)
    assert nh.min() > 500
    refs = [bowref.transform(ref, hd[f, :nh[f]], 2) for f in range(2)]
    for f in range(2):
        _assert_frame(hh, f, refs[f][0], refs[f][1])
    nn = out["n_nodes"].cpu().numpy()
    nodes = [(out["node_id"][f, :nn[f]], out["node_start"][f, :nn[f] + 1], out["feat"][f]) for f in range(2)]   # views of the transform's output, no conversion
    ang = [kps[f, :nh[f], 3].contiguous() for f in range(2)]
    has = torch.ones(int(nh[0]), dtype=torch.uint8, device="cuda")
    m = Matcher(max_keypoints=cap, max_mappoints=16)
    match = torch.full((1, cap), -7, dtype=torch.int32, device="cuda"); nm = torch.zeros(1, dtype=torch.int32, device="cuda")
    view = Matcher.bow_view(desc[0, :nh[0]], desc[1, :nh[1]], ang[0], ang[1], has, nodes[0], nodes[1])
    m.SearchByBoW([view], 0.7, True, match, cap, nm, s.cuda_stream)
    torch.cuda.synchronize()
    flat = [bowref.flatten(refs[f][0], refs[f][1], cap) for f in range(2)]
    rn = [(fl["node_id"][:fl["n_nodes"]], fl["node_start"][:fl["n_nodes"] + 1], fl["feat"]) for fl in flat]
    em, en = orc.search_by_bow(hd[0, :nh[0]], hd[1, :nh[1]], ang[0].cpu().numpy(), ang[1].cpu().numpy(), np.ones(nh[0], np.uint8), rn[0], rn[1], 0.7, True)
    assert int(nm[0]) == en and en > 50 and np.array_equal(match[0, :nh[1]].cpu().numpy(), em)


def test_cpp_mirror(tmp_path):
    """plf::ORBVocabulary through its reference-signature overload (std::vector<cv::Mat>, DBoW2::BowVector, DBoW2::FeatureVector, levelsup): tests/cpp/bow_driver.cpp
    built against tests/mock/ and run"""
    exe = build_driver("bow_driver", tmp_path, "-O1", "-g", "-Wall")
    ref = bowref.make_vocab(91, 10, 5, bowref.TF_IDF, bowref.L1_NORM, zero_share=0.05, dup_share=0.1, full=30)
    bowref.save_text(ref, str(tmp_path / "voc.txt"), trailing_blank_lines=1)
    d1 = bowref.make_descriptors(ref, 1, 900); d2 = np.concatenate([d1[:400], bowref.make_descriptors(ref, 2, 300)])
    d1.tofile(str(tmp_path / "desc1.u8")); d2.tofile(str(tmp_path / "desc2.u8"))
    run = subprocess.run([str(exe), str(tmp_path)], text=True, capture_output=True)
    assert run.returncode == 0 and "bow driver ok" in run.stdout, "driver failed (rc %d)\n%s\n%s" % (run.returncode, run.stdout, run.stderr[-2000:])
    get = lambda name, dt: np.fromfile(str(tmp_path / name), dt)
    b1, f1 = bowref.transform(ref, d1, 4); b2, _ = bowref.transform(ref, d2, 4)
    assert np.array_equal(get("out_bow_id.u32", np.uint32), np.array([w for w, _ in b1], np.uint32))
    assert np.array_equal(get("out_bow_val.f64", np.float64).view(np.uint64), np.array([v for _, v in b1]).view(np.uint64))
    fv_flat = []
    for nd, fs in f1:
        fv_flat += [nd, len(fs)] + fs
    assert np.array_equal(get("out_fv.u32", np.uint32), np.array(fv_flat, np.uint32))
    exp = np.array([bowref.score(ref.scoring, b1, b2), bowref.score(ref.scoring, b1, b1)])
    assert np.array_equal(get("out_score.f64", np.float64).view(np.uint64), exp.view(np.uint64)) and exp[0] > 0
