"""k_octree (DistributeOctTree): byte-equal to the oracle on small images that reach every branch of the kernel (tests/octree_cases.py) -- no candidates,
one candidate, ties in the best-key pass, a quota met exactly by phase 1, sweeps that stall, phase-2 sorts of 0, 1, 64 and more than 128 nodes and of
counts that are no power of two -- alone and in a batch.

Not covered, because no input reaches it: a level that ends with more nodes than its selection capacity (quota + 32, status bit 4).  The first sweep makes
at most 4 children of each of at most 8 roots = 32 nodes; any later sweep starts below the quota N, and either runs in phase 2, which stops at the first
node count >= N (at most N + 2), or in phase 1 with Lsz + 3 * expandable <= N, which cannot pass N.  The largest overshoot, 4 nodes for a quota of 1, is the
case "quota 1"."""
import numpy as np
import pytest

import orc
import octree_cases as oc

NL = oc.NLEVELS


def dots(seed, n):
    rng = np.random.default_rng(seed)
    img = np.full((oc.H, oc.W), 60, np.uint8)
    for x, y in zip(rng.integers(24, oc.W - 24, n), rng.integers(24, oc.H - 24, n)):
        img[y:y + 2, x:x + 2] = 230
    return img


def one_dot():
    img = np.full((oc.H, oc.W), 60, np.uint8)
    img[70:72, 90:92] = 230
    return img


# name -> (image, nfeatures); what each is for is asserted on the CPU in test_the_inputs_reach_every_situation
CASES = {
    "flat": (oc.flat, 40),
    "one dot": (one_dot, 40),
    "two-valued noise": (lambda: oc.two_level_noise(1), 40),
    "cluster": (lambda: oc.cluster(1), 40),
    "dots": (lambda: dots(0, 10), 40),
    "polygons": (lambda: oc.polygons(3), 40),
    "two-valued noise, 400": (lambda: oc.two_level_noise(1), 400),
    "noise, 400": (lambda: oc.noise(1), 400),
    "noise, 900": (lambda: oc.noise(1), 900),
    "quota 1": (lambda: oc.noise(1), 3),
    "noise, 40": (lambda: oc.noise(1), 40),
}
_REF = {}


def _ref(name):
    """image, oracle result with stages, per-level octree inputs and traces: computed once, never modified"""
    if name not in _REF:
        gen, nf = CASES[name]
        img = gen()
        lv, ref = oc.level_candidates(img, nf)
        trs = []
        for k, w_, h_, n in lv:
            sel, tr = oc.octree_schedule(k[:, 0].copy(), k[:, 1].copy(), k[:, 2].copy(), w_, h_, n)
            assert sel.tolist() == orc.distribute_octree(k, 16, 16 + w_, 16, 16 + h_, n)["class_id"].tolist()
            trs.append(tr)
        _REF[name] = (img, nf, lv, ref, trs)
    return _REF[name]


def _extractor(nf, max_batch=1):
    from rgbd_pl_slam_amd import ORBextractor
    return ORBextractor(nfeatures=nf, nlevels=NL, max_width=oc.W, max_height=oc.H, max_batch=max_batch)


def _check_frame(ext, frame, kps, desc, name):
    img, nf, lv, ref, trs = _ref(name)
    assert kps.tobytes() == ref["kps"].tobytes(), "key points of '%s'" % name
    assert np.array_equal(desc, ref["desc"]), "descriptors of '%s'" % name
    for l, (k, w_, h_, n) in enumerate(lv):
        cand = ext.candidates(frame, l)
        assert np.array_equal(cand, k), "octree input of '%s', level %d" % (name, l)
        out = orc.distribute_octree(cand, 16, 16 + w_, 16, 16 + h_, n)
        want = ref["level_kps"][l]
        assert int(np.sum(kps["octave"] == l)) == len(out) == len(want), "key points of '%s' in octave %d" % (name, l)
        for fld in ("x", "y"):
            assert np.array_equal(out[fld] + np.float32(16), want[fld]), "%s of '%s', octave %d" % (fld, name, l)
        assert np.array_equal(out["response"], want["response"]), "responses of '%s', octave %d" % (name, l)


def test_the_inputs_reach_every_situation():
    """on the CPU: what the oracle and the schedule model do on the inputs (pytest -s prints the candidate and node counts)"""
    t = {name: _ref(name)[4] for name in CASES}
    for name, trs in t.items():
        for l, tr in enumerate(trs):
            print("%-22s level %d: nk %5d, roots %d, nodes per sweep %s, phase-1 sweeps %d, sorts %s" % (name, l, tr["nk"], tr["roots"], tr["sizes"], tr["phase1"], tr["sorts"]))
    sorts = lambda name: [s for tr in t[name] for s in tr["sorts"]]
    assert [tr["nk"] for tr in t["flat"]] == [0, 0, 0]
    assert [tr["nk"] for tr in t["one dot"]] == [0, 1, 1] and t["one dot"][1]["stalled"] and t["one dot"][1]["sizes"] == [1]   # Lsz == prev at once
    assert [tr["nk"] for tr in t["two-valued noise"]] == [197, 26, 183]
    assert t["two-valued noise"][0]["exact_phase1"]                               # quota met exactly by phase 1
    resp = _ref("two-valued noise")[2][0][0][:, 2]
    assert len(np.unique(resp)) <= 4 and len(resp) == 197                          # few distinct responses: ties in the best-key pass
    no_retry = orc.orb_extract(_ref("two-valued noise")[0], nfeatures=40, nlevels=NL, ini_th=20, min_th=20)["ncand"]
    assert no_retry[0] < 197                                                        # the FAST retry with minThFAST found the rest
    assert all(tr["stalled"] and tr["sizes"][-1] == 4 for tr in t["cluster"])       # one cluster: the sweeps stop adding nodes below the quota
    assert 1 in sorts("dots") and 0 in sorts("dots")                                # a sort of one node, and a round with nothing left to divide
    assert 13 in sorts("polygons") and {50, 47, 29, 52} <= set(sorts("two-valued noise, 400"))   # not powers of two, below 64
    assert sorts("noise, 400") == [64, 64, 64]                                      # exactly one wave
    assert max(sorts("noise, 900")) > 128                                           # steps across waves (j = 64, 128)
    assert all(tr["sizes"] == [4] for tr in t["quota 1"])                           # 4 nodes for a quota of 1
    assert all(tr["phase1"] >= 1 and (tr["sorts"] or tr["exact_phase1"] or tr["stalled"]) for name in ("two-valued noise", "cluster", "polygons")
               for tr in t[name])                                                   # phase 2 (or an exact / stalled end) at every level


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_every_case_equals_the_oracle(name):
    ext = _extractor(CASES[name][1])
    kps, desc = ext(_ref(name)[0])
    _check_frame(ext, 0, kps, desc, name)
    ext.close()


@pytest.mark.gpu
def test_batch_of_three_and_the_same_images_alone():
    """cluster (89, 58, 40 keys), noise (1713, 951, 505), polygons (62, 50, 41) in one batch; the same images one at a time give the same bytes"""
    names = ["cluster", "noise, 40", "polygons"]
    imgs = np.stack([_ref(n)[0] for n in names])
    assert [[tr["nk"] for tr in _ref(n)[4]] for n in names] == [[89, 58, 40], [1713, 951, 505], [62, 50, 41]]
    ext = _extractor(40, max_batch=3)
    res = ext.extract_batch(imgs)
    for f, n in enumerate(names):
        _check_frame(ext, f, res[f][0], res[f][1], n)
    for f, n in enumerate(names):
        kps, desc = ext(imgs[f])
        assert kps.tobytes() == res[f][0].tobytes() and desc.tobytes() == res[f][1].tobytes(), "frame %d alone" % f
    ext.close()
