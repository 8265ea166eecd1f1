"""CPU tests of the track-to-detection association (include/pagk.h): the literal sequential restatement (tests/associate_ref.c:
the std::set and erase loop of MatchFeatures, the iterator loop of SearchByOpencvKLT) against an independent numpy model of
the count-and-compact formulation the device runs, byte for byte -- the proof that the device formulation is the
reference's --, with pagk_match_features and the oracle; the KLT arm on hand-built point sets that take every branch, on
the inputs the GPU tests use as well; the boundary (header, bindings, structure, argument checks that need no device)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import associate_ref_util as au
import lk_ref_util as lu
from pixel_aware_gyro_aided_klt_feature_tracker_amd import capi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("pagk_assoc_params_default", "pagk_assoc_params_check", "pagk_match_features_device",
                "pagk_search_gyro_predict_device", "pagk_search_gyro_predict", "pagk_search_klt_device", "pagk_search_klt")
F = np.float32


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return au.build_ref(tmp_path_factory.mktemp("associate_ref"))


@pytest.fixture(scope="module")
def lk(tmp_path_factory):
    return lu.build_ref(tmp_path_factory.mktemp("lk_ref_for_associate"))


# ---- the boundary --------------------------------------------------------------------------------------------------------
def test_header_declares_and_capi_binds_the_entry_points(built):
    hdr = open(os.path.join(ROOT, "include", "pagk.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = capi.load()
    for name in ENTRY_POINTS:
        assert name in capi.EXPORTED_SYMBOLS and hasattr(lib, name) and getattr(lib, name).argtypes, name
        assert re.search(r"\b(?:int|void) " + name + r"\s*\(", code), name
        decl = re.search(r"\b(?:int|void) " + name + r"\(", hdr).start()       # every declaration cites the reference lines
        comment = hdr[:decl].rsplit("/*", 1)[1]
        assert "src/gyro_aided_tracker.cpp:" in comment and comment.rstrip().endswith("*/"), name
    begin = hdr[hdr.index("hipGraph capture of the per-frame work"):hdr.index("int pagk_graph_begin")]
    for name in ("pagk_match_features_device", "pagk_search_gyro_predict_device", "pagk_search_klt_device"):
        assert name in begin, name
    for word in ("Track-to-detection association", "NOT claimed", "tests/associate_ref.c", "the library's own rule",
                 "tie order of equal distances", "`<=` at the radius", "over-long lists", "exactly one feature"):
        assert word in hdr, word
    assert "sequential by nature" not in hdr
    assert [f[0] for f in capi.AssocParams._fields_] == ["th_ncc_high", "th_ncc_low", "th_ratio", "use_ncc", "min_matches",
                                                         "klt_max_distance", "klt_ratio", "klt_disparity_factor"]
    assert C.sizeof(capi.AssocParams) == 40 and capi.AssocParams.klt_ratio.offset == 24
    assert capi.ASSOC_INFO_WORDS == 8 == int(re.search(r"#define PAGK_ASSOC_INFO_WORDS (\d+)", hdr).group(1))
    assert capi.ASSOC_STATS_WORDS == 8 == int(re.search(r"#define PAGK_ASSOC_STATS_WORDS (\d+)", hdr).group(1))
    d = capi.assoc_params_default()
    assert (d.th_ncc_high, d.th_ncc_low, d.th_ratio) == (F(0.6), F(0.3), F(0.75))
    assert (d.use_ncc, d.min_matches, d.klt_max_distance, d.klt_ratio, d.klt_disparity_factor) == (1, 100, 4.0, 0.7, 1.5)
    for meth in ("match_features_device", "search_gyro_predict_device", "search_gyro_predict", "search_klt_device", "search_klt"):
        assert callable(getattr(capi.Context, meth))
    from pixel_aware_gyro_aided_klt_feature_tracker_amd import host_api
    assert callable(host_api.search_by_gyro_predict) and callable(host_api.search_by_klt)


def test_params_check_refuses_each_bad_field(built):
    assert capi.assoc_params_check(capi.assoc_params_default()) == capi.PAGK_OK
    assert capi.assoc_params_check(capi.assoc_params_default(th_ncc_high=0.0, th_ncc_low=0.0, th_ratio=0.0, use_ncc=0,
                                                             min_matches=0, klt_max_distance=0.0, klt_ratio=0.0,
                                                             klt_disparity_factor=0.0)) == capi.PAGK_OK
    for field in ("th_ncc_high", "th_ncc_low", "th_ratio", "klt_max_distance", "klt_ratio", "klt_disparity_factor"):
        for v in (-1e-6, float("nan"), float("inf")):
            assert capi.assoc_params_check(capi.assoc_params_default(**{field: v})) == capi.PAGK_E_ARG, (field, v)
    for kw in (dict(use_ncc=2), dict(use_ncc=-1), dict(min_matches=-1)):
        assert capi.assoc_params_check(capi.assoc_params_default(**kw)) == capi.PAGK_E_ARG, kw
    assert capi.load().pagk_assoc_params_check(None) == capi.PAGK_E_ARG
    with pytest.raises(TypeError):
        capi.assoc_params_default(radius=3)


def test_every_entry_point_refuses_without_a_context(built):
    lib = capi.load()
    ap, lp = capi.assoc_params_default(), capi.lk_params_default()
    buf = np.zeros(64, np.float64)
    a = buf.ctypes.data
    img = capi.image_view(np.zeros((64, 64), np.uint8))
    E = capi.PAGK_E_ARG
    assert lib.pagk_match_features_device(None, C.byref(ap), 1, 1, 1, a, a, a, a, a, a, None, None, a, a) == E
    assert lib.pagk_search_gyro_predict_device(None, C.byref(ap), 0, 1, 5, 1, a, a, a, None, 1, a, a, None, 10.0, 4, a, a, a, a,
                                               a, a, None, None, a, None, a) == E
    assert lib.pagk_search_gyro_predict(None, C.byref(ap), C.byref(img), C.byref(img), 5, 1, a, a, a, None, 1, a, a, 10.0, 4, a,
                                        a, a, a, a, a, None, None, None, None) == E
    assert lib.pagk_search_klt_device(None, C.byref(lp), C.byref(ap), 0, 1, 4, a, None, 1, a, None, a, a, a, a, a, None, a, a, a,
                                      a, a) == E
    assert lib.pagk_search_klt(None, C.byref(lp), C.byref(ap), C.byref(img), C.byref(img), 1, a, 1, a, a, a, a, a, a, None, a,
                                None, None, None) == E


# ---- MatchFeatures: the sequential pass is a count and a compaction ----------------------------------------------------------
@pytest.mark.parametrize("use_ncc", [True, False])
@pytest.mark.parametrize("cap", [1, 2, 8])
@pytest.mark.parametrize("m", [1, 3, 17])
def test_sequential_restatement_equals_count_and_compact(built, ref, m, cap, use_ncc):
    from oracle import pagk_oracle as orc
    seen = np.zeros(4, np.int64)          # current keypoints claimed 0, 1, 2 and 3 or more times
    for seed, n in enumerate((0, 1, 5, 40, 300)):
        rng = np.random.default_rng(1000 + seed)
        count, idx, dist, ncc = au.random_lists(0xA550C + 16 * seed + m + cap, n, m, cap)
        cur, pred = rng.uniform(0, 100, (max(m, 1), 2)).astype(F), rng.uniform(0, 100, (max(n, 1), 2)).astype(F)
        r = au.ref_match(ref, count, idx, dist, ncc, m, use_ncc, keys_cur_un=cur, pt_pred=pred)
        mo = au.model_match(count, idx, dist, ncc, m, use_ncc, keys_cur_un=cur, pt_pred=pred)
        assert au.differing(r, mo, au.MATCH_KEYS) == [], (n, m, cap, use_ncc)
        k = int(r["k"])
        for got in (capi.match_features(count, idx, dist, ncc, use_ncc), orc.match_features(count, idx, dist, ncc, use_ncc)):
            assert len(got[0]) == k
            for a, b in zip(got, (r["query"], r["train"], r["dist"], r["ncc"])):
                assert au.same_array(a, b[:k]), (n, m, cap, use_ncc)
        # how often each current keypoint was claimed, from the model's own choice rule
        claims = np.bincount(idx[:, 0][_chosen(count, idx, dist, ncc, cap, use_ncc)], minlength=m) if n else np.zeros(m, int)
        for c in range(4):
            seen[c] += int((np.minimum(claims, 3) == c).sum())
        # over-long lists and indices out of range: the library's own rule, the restatement and the model agree
        c2, i2, d2, n2 = au.random_lists(0xBAD + seed + m + cap, n, m, cap, overlong=True, bad_index=True)
        r2, m2 = au.ref_match(ref, c2, i2, d2, n2, m, use_ncc), au.model_match(c2, i2, d2, n2, m, use_ncc)
        assert au.differing(r2, m2, au.MATCH_KEYS) == []
        if n >= 40:
            assert r2["info"][1] > 0
    if m == 17:
        assert seen.min() > 0, seen       # claimed 0, 1, 2 and >= 3 times
    else:
        assert seen[3] > 0 and seen[1:].sum() > 0, seen


def _chosen(count, idx, dist, ncc, cap, use_ncc):
    """Rows with a choice, by a plain loop over the rule of src/gyro_aided_tracker.cpp:955-990."""
    out = []
    for i, c in enumerate(count.tolist()):
        if c <= 0 or c > cap:
            continue
        if use_ncc:
            if ncc[i, 0] > F(0.6):
                out.append(i)
            elif c > 1 and not ncc[i, 0] < F(0.3) and ncc[i, 1] < F(ncc[i, 0] * F(0.75)):
                out.append(i)
        elif c == 1 or dist[i, 0] < F(dist[i, 1] * F(0.75)):
            out.append(i)
    return np.array(out, np.int64)


def test_nan_and_infinite_scores_are_among_the_lists():
    count, idx, dist, ncc = au.random_lists(0xA550C + 3 + 17 + 8, 300, 17, 8)
    assert np.isnan(ncc).any() and np.isposinf(ncc).any() and np.isneginf(ncc).any()
    assert np.isnan(dist).any() and np.isposinf(dist).any() and np.isneginf(dist).any()
    assert np.isnan(ncc[:, 0]).any() or np.isnan(ncc[:, 1]).any()


def test_match_by_hand(ref):
    # features 0 and 2 choose keypoint 1 (both lose it, and feature 4, which comes later, does not get it either);
    # feature 1 alone chooses keypoint 0; feature 3 has two similar scores; feature 5 a low best score
    count = np.array([1, 1, 2, 2, 1, 2], np.int32)
    idx = np.array([[1, 0], [0, 0], [1, 2], [2, 0], [1, 0], [2, 1]], np.int32)
    ncc = np.array([[.9, 0], [.7, 0], [.5, .1], [.5, .45], [.8, 0], [.2, .01]], F)
    dist = np.ones((6, 2), F)
    r = au.ref_match(ref, count, idx, dist, ncc, 3)
    assert int(r["k"]) == 1 and r["query"].tolist() == [1, -1, -1, -1, -1, -1] and r["train"][0] == 0
    assert r["info"].tolist() == [4, 0, 0, 1, 1, 0, 0, 0]
    assert au.differing(r, au.model_match(count, idx, dist, ncc, 3), au.MATCH_KEYS) == []


# ---- the KLT arm ---------------------------------------------------------------------------------------------------------
def test_klt_hand_built_set_takes_every_branch(ref):
    status, pl, pr, n, cap = au.synthetic_queries()
    keys, used = au.branch_keypoints(pl, status, pr, n)
    assert list(used) == list(au.SCENARIOS)
    r = au.ref_klt(ref, cap, n, status, pl, pr, keys)
    assert au.differing(r, au.model_klt(cap, n, status, pl, pr, keys), au.KLT_KEYS) == []
    k = int(r["k"])
    q = r["query"][:k].tolist()
    # 11 live queries: "none" and "beyond 4" have no neighbour; "at 4", "inside 4" and the three of the cluster have one
    assert r["info"][:6].tolist() == [11, 2, 5, 4, 3, 2]
    survivors_before_filter = [used["at 4"], used["inside 4"], used["ratio below"], used["three"][0]]
    assert int(r["info"][6]) + k == len(survivors_before_filter) and set(q) <= set(survivors_before_filter)
    assert used["ratio below"] in q and used["three"][0] in q          # small disparities: kept
    assert used["ratio above"] not in q and used["equal pair"] not in q and used["two at 0"] not in q
    assert used["three"][1] not in q and used["three"][2] not in q     # lost to the earlier claimer
    i = used["ratio below"]
    row = q.index(i)
    d0 = r["dist"][row]
    assert d0 == F(2) * au.R_BELOW and np.float64(d0 / F(2)) < 0.7 <= np.float64(F(2) * au.R_ABOVE / F(2))
    # the neighbour at exactly 4.0f is a neighbour; one ulp further it is not
    assert F(4.0) in au._dist(pl[used["at 4"]], keys)
    assert np.nextafter(F(4), F(5), dtype=F) in au._dist(pl[used["beyond 4"]], keys)
    assert np.nextafter(F(4), F(0), dtype=F) in au._dist(pl[used["inside 4"]], keys)
    assert (au._dist(pl[used["two at 0"]], keys) == 0).sum() == 2
    assert (au._dist(pl[used["equal pair"]], keys) == F(1.5)).sum() == 2
    # equal distances keep the lower train index in front: with a ratio that accepts a tie the lower index is the match
    tie = au.ref_klt(ref, cap, n, status, pl, pr, keys, ratio=1.5)
    row = tie["query"].tolist().index(used["equal pair"])
    pair = np.flatnonzero(au._dist(pl[used["equal pair"]], keys) == F(1.5))
    assert tie["train"][row] == pair.min()
    assert au.differing(tie, au.model_klt(cap, n, status, pl, pr, keys, ratio=1.5), au.KLT_KEYS) == []


def test_klt_disparity_filter_drops_some_none_and_all_but_one(ref):
    status, pl, pr, n, cap = au.synthetic_queries()
    sets = au.klt_sets(pl, status, pr, n)
    r = {name: au.ref_klt(ref, cap, n, status, pl, pr, keys) for name, keys in sets.items()}
    for name, keys in sets.items():
        assert au.differing(r[name], au.model_klt(cap, n, status, pl, pr, keys), au.KLT_KEYS) == [], name
    assert r["branches"]["info"][6] >= 1 and r["branches"]["info"][7] >= 1                 # some
    assert r["exact"]["info"][6] == 0 and r["exact"]["info"][7] == r["exact"]["info"][0]   # none: every live query matched
    assert r["two"]["info"][6] == 1 and r["two"]["info"][7] == 1                           # all but one
    z = r["empty"]
    assert z["info"].tolist() == [11, 11, 0, 0, 0, 0, 0, 0] and int(z["k"]) == 0           # zero matches: avg is NaN
    assert np.isnan(z["stats"][0]) and np.isnan(z["stats"][1]) and np.isnan(z["stats"][4]) and z["stats"][5] == 0
    assert np.all(z["query"] == -1) and not z["disparity"].any()
    dead = au.ref_klt(ref, cap, n, np.zeros(cap, np.uint8), pl, pr, sets["exact"])         # all statuses 0
    assert dead["info"].tolist() == [0] * 8 and np.isnan(dead["stats"][0])


@pytest.fixture(scope="module")
def gpu_inputs(lk):
    """The inputs of the GPU tests' KLT cases: Lucas-Kanade's outputs by its restatement, and the sets built from them."""
    out = {}
    for name, c in au.klt_cases(synth).items():
        t = lu.ref_track(lk, c["ref"], c["cur"], c["pts"], c["p"], c["cap"], c["n"])
        pr = np.zeros((c["cap"], 2), F)
        pr[:len(c["pts"])] = c["pts"]
        out[name] = (c, t, pr, au.klt_sets(t["pt_out"], t["status"], pr, c["n"]))
    return out


def test_every_branch_is_reached_on_the_inputs_of_the_gpu_tests(ref, gpu_inputs):
    total = np.zeros(au.INFO_WORDS, np.int64)
    none_dropped = all_but_one = zero = dead = 0
    for name, (c, t, pr, sets) in gpu_inputs.items():
        keys, used = au.branch_keypoints(t["pt_out"], t["status"], pr, c["n"])
        assert list(used) == list(au.SCENARIOS), (name, list(used))
        assert set(sets) == {"branches", "exact", "empty", "two"}, name
        for kind, keys in sets.items():
            r = au.ref_klt(ref, c["cap"], c["n"], t["status"], t["pt_out"], pr, keys)
            assert au.differing(r, au.model_klt(c["cap"], c["n"], t["status"], t["pt_out"], pr, keys), au.KLT_KEYS) == [], (name, kind)
            print(name, kind, r["info"].tolist(), r["stats"][:5].tolist())
            total += r["info"]
            none_dropped += int(r["info"][6] == 0 and r["info"][7] >= 2)
            all_but_one += int(r["info"][6] >= 1 and r["info"][7] == 1)
            zero += int(r["info"][7] == 0 and np.isnan(r["stats"][0]))
        b = au.ref_klt(ref, c["cap"], c["n"], t["status"], t["pt_out"], pr, sets["branches"])["info"]
        assert b[1] >= 2 and b[2] >= 2 and b[3] >= 4 and b[4] >= 3 and b[5] >= 2, (name, b.tolist())
        dead += c["n"] - int(t["status"][:c["n"]].sum())
    assert np.all(total > 0), total.tolist()                              # no branch count is zero
    assert none_dropped >= 1 and all_but_one >= 1 and zero >= 1 and total[6] >= 2
    assert dead >= 1                                                      # live rows whose status the err filter cleared


# ---- sanitizers ----------------------------------------------------------------------------------------------------------
def test_restatement_runs_clean_under_the_sanitizers(tmp_path):
    """A stand-alone program (tests/associate_sanitize.c: its own main, compiled together with tests/associate_ref.c) runs both
    restatements on seeded inputs under AddressSanitizer and UBSan, every array in a heap block of exactly its size."""
    exe = str(tmp_path / "associate_sanitize")
    subprocess.run(["gcc", "-std=c99", "-O1", "-g", "-ffp-contract=off", "-fno-fast-math", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", os.path.join(ROOT, "tests", "associate_sanitize.c"),
                    os.path.join(ROOT, "tests", "associate_ref.c"), "-o", exe, "-lm"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "12 runs" in r.stdout, r.stdout
