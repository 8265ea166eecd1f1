"""GPU tests of the ORB descriptors and the matcher: pagk_orb_describe[_device] and pagk_orb_match[_device] against the
plain-C restatement (tests/orb_ref.c), byte for byte; describe on the detector's device output; capture and replay of
detect -> describe on two slots -> match; the host forms and host_api; the argument checks on a live context."""
import numpy as np
import pytest
import torch

import fast_ref_util as fu
import orb_ref_util as ou
from pixel_aware_gyro_aided_klt_feature_tracker_amd import capi, host_api, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return ou.build_ref(tmp_path_factory.mktemp("orb_ref"))


@pytest.fixture(scope="module")
def fref(tmp_path_factory):
    return fu.build_ref(tmp_path_factory.mktemp("fast_ref"))


@pytest.fixture(scope="module")
def images():
    return ou.images(synth)


@pytest.fixture(scope="module")
def restated(ref, images):
    """(pattern, count, weights) -> the restatement on the 97 x 80 image with cap = 300, computed once and left unchanged."""
    memo = {}

    def get(pattern, n, weights=ou.DEFAULT_WEIGHTS):
        key = (pattern, n, weights)
        if key not in memo:
            img = images["97x80 texture"]
            memo[key] = ou.ref_describe(ref, img, PATTERNS[pattern](), ou.many_keypoints(97, 80, 300), weights, cap=300, n=n)
        return memo[key]
    return get


PATTERNS = {"seeded": ou.seeded_pattern, "corners": ou.corner_pattern}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _set_slot(ctx, slot, img, pitch=None):
    """The image into a frame slot: uploaded, or read in place from the left columns of a wider device buffer (returned:
    the caller keeps it alive while the slot is used)."""
    h, w = img.shape
    if pitch is None:
        ctx.frame_upload(slot, img, 1)
        return None
    keep = torch.full((h, pitch), 255, dtype=torch.uint8, device=DEV)
    keep[:, :w] = _dev(img)
    torch.cuda.synchronize()
    ctx.frame_set_device(slot, keep.data_ptr(), w, h, pitch, 1)
    return keep


def _device_describe(ctx, img, pattern, kp, n, cap, weights=ou.DEFAULT_WEIGHTS, slot=2, pitch=None, with_angle=True):
    keep = _set_slot(ctx, slot, img, pitch)
    ctx.orb_set_pattern(pattern)
    buf = np.full((cap, 2), 1e9, np.float32)               # entries beyond the list are never read as coordinates that matter
    buf[:len(kp)] = kp
    d_k, d_n = _dev(buf), _dev(np.array([n], np.int32))
    d_a = torch.full((cap,), -7.0, dtype=torch.float32, device=DEV) if with_angle else None
    d_d = torch.full((cap, 32), 0x5a, dtype=torch.uint8, device=DEV)
    d_i = torch.full((capi.ORB_INFO_WORDS,), -7, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    ctx.orb_describe_device(capi.orb_params_default(blur_weights=weights), slot, cap, d_k, d_n, d_a, d_d, d_i)
    ctx.sync()
    out = dict(desc=d_d.cpu().numpy(), info=d_i.cpu().numpy(), angle=d_a.cpu().numpy() if with_angle else None)
    del keep
    return out


# ---- describe ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", ["seeded", "corners"])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_describe_device_form(ctx, ref, images, restated, pattern, n):
    img = images["97x80 texture"]
    kp = ou.many_keypoints(97, 80, 300)
    got = _device_describe(ctx, img, PATTERNS[pattern](), kp, n, 300, pitch=97 + 37)      # every output pre-filled
    want = restated(pattern, n)
    print(f"{pattern}, n = {n}: info {got['info'][:2].tolist()} (restated {want['info'][:2].tolist()})")
    assert ou.same(got, want, ou.DESC_KEYS) == []
    assert not got["desc"][n:].any() and not got["angle"][n:].any()                   # the tail is zeroed
    assert int(want["info"][0]) + int(want["info"][1]) == n
    if n == 257:
        assert want["info"][0] > 150 and want["info"][1] > 20
        # the border cases by name: 19 and W - 20 are described, 18 and W - 19 flagged, 20.5 -> 20 and 21.5 -> 22
        a = got["angle"]
        assert (a[:4] >= 0).all() and (a[4:8] == -1).all() and a[8] >= 0 and a[10] == -1 and a[11] >= 0 and (a[14:17] == -1).all()
        tie = ou.ref_describe(ref, img, PATTERNS[pattern](), np.array([[20, 22], [22, 20]], np.float32))
        assert got["desc"][8:10].tobytes() == tie["desc"].tobytes()


def test_describe_other_weights_no_angle_and_upload(ctx, images, restated):
    img = images["97x80 texture"]
    kp = ou.many_keypoints(97, 80, 300)
    wts = (70, 42, 33, 18)
    got = _device_describe(ctx, img, ou.seeded_pattern(), kp, 257, 300, weights=wts, with_angle=False)     # an uploaded slot
    want = restated("seeded", 257, wts)
    assert got["desc"].tobytes() == want["desc"].tobytes() and got["info"].tobytes() == want["info"].tobytes()
    assert want["desc"].tobytes() != restated("seeded", 257)["desc"].tobytes()              # the weights matter
    # twice the same bytes
    again = _device_describe(ctx, img, ou.seeded_pattern(), kp, 257, 300, weights=wts, with_angle=False)
    assert again["desc"].tobytes() == got["desc"].tobytes()


def test_describe_flat_edges_and_octants(ctx, ref, images):
    pat = ou.seeded_pattern()
    kp = np.array([[48, 40], [30, 40], [48, 25], [60.5, 40.5], [48, 39], [47, 40], [40, 33]], np.float32)
    for name in ["flat", "horizontal step", "vertical step"] + [f"gradient octant {k}" for k in range(8)]:
        got = _device_describe(ctx, images[name], pat, kp, len(kp), 8)
        assert ou.same(got, ou.ref_describe(ref, images[name], pat, kp, cap=8), ou.DESC_KEYS) == [], name


def test_describe_on_the_detectors_device_output(ctx, ref, fref, images):
    """detect -> describe with no host round trip: the detector's keypoint buffer and its info word 0 are the describe
    call's list and count."""
    img = images["160x120 texture"]
    n_features = 100
    cap = capi.detect_fast_bounds(160, 120, n_features)[1]
    pat = ou.seeded_pattern()
    ctx.frame_upload(1, img, 1)
    ctx.orb_set_pattern(pat)
    d_k = torch.full((cap, 2), -7.0, dtype=torch.float32, device=DEV)
    d_i = torch.full((8,), -7, dtype=torch.int32, device=DEV)
    d_a = torch.full((cap,), -7.0, dtype=torch.float32, device=DEV)
    d_d = torch.full((cap, 32), 0x5a, dtype=torch.uint8, device=DEV)
    d_oi = torch.full((8,), -7, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    ctx.detect_fast_device(capi.fast_params_default(n_features=n_features), 1, None, cap, d_k, None, d_i)
    ctx.orb_describe_device(capi.orb_params_default(), 1, cap, d_k, d_i, d_a, d_d, d_oi)
    ctx.sync()
    det = fu.ref_detect(fref, img, None, n_features)
    assert d_k.cpu().numpy().tobytes() == det["keypoints"].tobytes() and det["n"] > 30
    want = ou.ref_describe(ref, img, pat, det["keypoints"], cap=cap, n=det["n"])
    got = dict(angle=d_a.cpu().numpy(), desc=d_d.cpu().numpy(), info=d_oi.cpu().numpy())
    print(f"detect -> describe: {det['n']} keypoints, info {got['info'][:2].tolist()}")
    assert ou.same(got, want, ou.DESC_KEYS) == []
    assert got["info"][0] == det["n"] and got["info"][1] == 0            # the detector never leaves the border
    # host_api.orb_extract is the same composition on host arrays
    ex = host_api.orb_extract(img, n_features, pat, ctx=ctx)
    assert ex["keypoints"].tobytes() == det["keypoints"][:det["n"]].tobytes()
    assert ex["desc"].tobytes() == want["desc"][:det["n"]].tobytes() and ex["angle"].tobytes() == want["angle"][:det["n"]].tobytes()


# ---- match -------------------------------------------------------------------------------------------------------------
def _device_match(ctx, dq, dt, nq, nt, cap_q, cap_t, match_floor=30):
    bq, bt = np.full((cap_q, 32), 0xa5, np.uint8), np.full((cap_t, 32), 0x3c, np.uint8)
    bq[:len(dq)], bt[:len(dt)] = dq, dt
    d_q, d_t, d_c = _dev(bq), _dev(bt), _dev(np.array([nq, nt], np.int32))
    d_idx = torch.full((cap_q,), -7, dtype=torch.int32, device=DEV)
    d_dist = torch.full((cap_q,), -7, dtype=torch.int32, device=DEV)
    d_keep = torch.full((cap_q,), 7, dtype=torch.uint8, device=DEV)
    d_i = torch.full((capi.ORB_INFO_WORDS,), -7, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    ctx.orb_match_device(capi.orb_params_default(match_floor=match_floor), cap_q, d_q, d_c[0:1], cap_t, d_t, d_c[1:2], d_idx,
                         d_dist, d_keep, d_i)
    ctx.sync()
    return dict(train_idx=d_idx.cpu().numpy(), distance=d_dist.cpu().numpy(), keep=d_keep.cpu().numpy(), info=d_i.cpu().numpy())


def _match_case(name):
    """-> (query rows, train rows, what the case is known to give: {query: train index})."""
    if name == "0 x 5":
        return ou.random_descriptors(0, 1), ou.random_descriptors(5, 2), {}
    if name == "5 x 0":
        return ou.random_descriptors(5, 1), ou.random_descriptors(0, 2), {}
    if name == "1 x 1":
        t = ou.random_descriptors(1, 3)
        return np.bitwise_not(t), t, {0: 0}
    if name == "70 x 130":
        q, t = ou.random_descriptors(70, 4), ou.random_descriptors(130, 5)
        t[129] = t[0]                                   # a duplicate at the lowest and the highest index
        q[7], q[69] = t[129], ou.flip_bits(t[129], 2, 1)
        q[64] = ou.flip_bits(t[128], 4, 2)              # past the first query wave, in the second train chunk
        return q, t, {7: 0, 69: 0, 64: 128}
    if name == "33 x 1025":
        q, t = ou.random_descriptors(33, 6), ou.random_descriptors(1025, 7)
        known = {0: 1024, 20: 1}
        t[1000] = t[1]                                  # a duplicate pair seven chunks apart
        q[20] = t[1000]
        q[0] = ou.flip_bits(t[1024], 3, 1)              # the best train row is the last one, alone in its chunk
        for k, b in enumerate(range(128, 1025, 128)):   # one on each side of every chunk boundary
            q[1 + 2 * k], q[2 + 2 * k] = ou.flip_bits(t[b - 1], 5, k), ou.flip_bits(t[b], 6, k)
            known[1 + 2 * k], known[2 + 2 * k] = b - 1, b
        return q, t, known
    if name == "3 x 65700":                             # beyond 512 chunks: a workgroup walks more than one
        q, t = ou.random_descriptors(3, 8), ou.random_descriptors(65700, 9)
        q[0], q[1], q[2] = ou.flip_bits(t[65699], 1, 1), ou.flip_bits(t[65536], 2, 2), ou.flip_bits(t[127], 3, 3)
        return q, t, {0: 65699, 1: 65536, 2: 127}
    raise KeyError(name)


@pytest.mark.parametrize("name", ["0 x 5", "5 x 0", "1 x 1", "70 x 130", "33 x 1025", "3 x 65700"])
def test_match_device_form(ctx, ref, name):
    q, t, known = _match_case(name)
    nq, nt = len(q), len(t)
    cap_q, cap_t = max(nq, 1) + 3, max(nt, 1) + 2         # capacities above the counts: the padding rows are never matched
    got = _device_match(ctx, q, t, nq, nt, cap_q, cap_t)
    want = ou.ref_match(ref, q, t, cap_q=cap_q)
    print(f"{name}: info {got['info'][:6].tolist()} (restated {want['info'][:6].tolist()})")
    assert ou.same(got, want, ou.MATCH_KEYS) == []
    for k, v in known.items():
        assert got["train_idx"][k] == v, (name, k)
    assert (got["train_idx"][nq:] == -1).all() and (got["distance"][nq:] == 257).all() and not got["keep"][nq:].any()
    again = _device_match(ctx, q, t, nq, nt, cap_q, cap_t)
    assert ou.same(again, got, ou.MATCH_KEYS) == []         # the same bytes twice, whatever order the atomics took
    if name == "70 x 130":                                  # a count below the rows present, another floor
        got = _device_match(ctx, q, t, 66, 129, cap_q, cap_t, match_floor=120)
        want = ou.ref_match(ref, q, t, match_floor=120, cap_q=cap_q, nq=66, nt=129)
        assert ou.same(got, want, ou.MATCH_KEYS) == [] and got["info"][5] == 120 and got["keep"][:66].sum() > 3


# ---- the host forms ----------------------------------------------------------------------------------------------------
def test_host_forms_equal_the_device_forms(ctx, ref, images, restated):
    img = images["97x80 texture"]
    kp = ou.many_keypoints(97, 80, 300)[:257]
    ctx.orb_set_pattern(ou.seeded_pattern())
    got, want = ctx.orb_describe(img, kp), restated("seeded", 257)
    assert got["desc"].tobytes() == want["desc"][:257].tobytes() and got["angle"].tobytes() == want["angle"][:257].tobytes()
    assert got["info"].tobytes() == want["info"].tobytes() and (got["described"], got["outside"]) == tuple(want["info"][:2])
    empty = ctx.orb_describe(img, np.zeros((0, 2), np.float32))
    assert empty["desc"].shape == (0, 32) and empty["info"].tolist() == [0] * 8
    for name in ("0 x 5", "5 x 0", "70 x 130", "33 x 1025"):
        q, t, _ = _match_case(name)
        got, want = ctx.orb_match(q, t), ou.ref_match(ref, q, t)
        n = len(q)
        assert got["info"].tobytes() == want["info"].tobytes(), name
        for k in ("train_idx", "distance", "keep"):
            assert got[k].tobytes() == want[k][:n].tobytes(), (name, k)
    # FindFeatureMatches on a pair: an image and itself moved by (+3, +2)
    import detect_ref_util as du
    base = du.texture_image(synth, 200, 160, 21)
    pair = host_api.orb_match_pair(np.ascontiguousarray(base[10:130, 10:170]), np.ascontiguousarray(base[8:128, 7:167]), 60,
                                   ou.seeded_pattern(), ctx=ctx)
    want = ou.ref_match(ref, pair["ref"]["desc"], pair["cur"]["desc"])
    assert pair["info"].tobytes() == want["info"].tobytes() and pair["nq"] == len(pair["ref"]["keypoints"]) > 20
    assert pair["train_idx"].tobytes() == want["train_idx"][:pair["nq"]].tobytes()
    moved = pair["cur"]["keypoints"][pair["train_idx"]] - pair["ref"]["keypoints"]
    exact = (pair["distance"] == 0) & pair["keep"].astype(bool)
    print(f"pair: {pair['nq']} keypoints, {pair['kept']} kept, {int(exact.sum())} with distance 0")
    assert exact.sum() > 5 and (moved[exact] == np.array([3, 2], np.float32)).all()


# ---- capture -----------------------------------------------------------------------------------------------------------
def test_capture_detect_describe_match_and_replay(ref, fref):
    import detect_ref_util as du
    w, h, n_features = 160, 120, 80
    frames = [du.texture_image(synth, w, h, s) for s in (12, 13, 14, 15)]
    pairs = [(0, 1), (2, 3), (1, 2)]
    cap = capi.detect_fast_bounds(w, h, n_features)[1]
    pat = ou.seeded_pattern()
    fast, orb = capi.fast_params_default(n_features=n_features), capi.orb_params_default()
    c = capi.Context(0)
    try:
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            c.set_stream(stream.cuda_stream)
            c.orb_set_pattern(pat)
            d_img = [torch.zeros((h, w), dtype=torch.uint8, device=DEV) for _ in range(2)]
            z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=DEV)
            d_k = [z((cap, 2), torch.float32) for _ in range(2)]
            d_di = [z(8, torch.int32) for _ in range(2)]
            d_a = [z(cap, torch.float32) for _ in range(2)]
            d_d = [z((cap, 32), torch.uint8) for _ in range(2)]
            d_oi = [z(8, torch.int32) for _ in range(2)]
            d_idx, d_dist, d_keep, d_mi = z(cap, torch.int32), z(cap, torch.int32), z(cap, torch.uint8), z(8, torch.int32)

            def work():
                for s in range(2):
                    c.frame_set_device(s, d_img[s].data_ptr(), w, h, w, 1)
                    c.detect_fast_device(fast, s, None, cap, d_k[s], None, d_di[s])
                    c.orb_describe_device(orb, s, cap, d_k[s], d_di[s], d_a[s], d_d[s], d_oi[s])
                c.orb_match_device(orb, cap, d_d[0], d_di[0], cap, d_d[1], d_di[1], d_idx, d_dist, d_keep, d_mi)

            def snapshot():
                stream.synchronize()
                return [t.cpu().numpy().tobytes() for t in d_k + d_a + d_d + d_oi + [d_idx, d_dist, d_keep, d_mi]]

            def feed(pair):
                for s in range(2):
                    d_img[s].copy_(_dev(frames[pair[s]]))

            def check(pair, how):
                want_d = []
                for s in range(2):
                    det = fu.ref_detect(fref, frames[pair[s]], None, n_features)
                    want_d.append((det, ou.ref_describe(ref, frames[pair[s]], pat, det["keypoints"], cap=cap, n=det["n"])))
                    assert d_d[s].cpu().numpy().tobytes() == want_d[s][1]["desc"].tobytes(), (how, pair, s)
                    assert d_a[s].cpu().numpy().tobytes() == want_d[s][1]["angle"].tobytes(), (how, pair, s)
                    assert d_oi[s].cpu().numpy().tobytes() == want_d[s][1]["info"].tobytes(), (how, pair, s)
                m = ou.ref_match(ref, want_d[0][1]["desc"], want_d[1][1]["desc"], cap_q=cap, nq=want_d[0][0]["n"],
                                 nt=want_d[1][0]["n"])
                got = dict(train_idx=d_idx.cpu().numpy(), distance=d_dist.cpu().numpy(), keep=d_keep.cpu().numpy(),
                           info=d_mi.cpu().numpy())
                print(f"{how} {pair}: match info {got['info'][:6].tolist()}")
                assert ou.same(got, m, ou.MATCH_KEYS) == [], (how, pair)

            direct = {}
            for pair in pairs:                        # the direct calls (the first one sizes every workspace)
                feed(pair)
                work()
                direct[pair] = snapshot()
                check(pair, "direct")
            c.graph_begin()
            try:
                with pytest.raises(capi.PagkError):   # the host-buffer forms are not capturable
                    c.orb_describe(frames[0], np.zeros((1, 2), np.float32))
                with pytest.raises(capi.PagkError):
                    c.orb_match(np.zeros((1, 32), np.uint8), np.zeros((1, 32), np.uint8))
                with pytest.raises(capi.PagkError):
                    c.orb_set_pattern(pat)
                work()
            finally:
                gid = c.graph_end()
            for pair in (pairs[1], pairs[2], pairs[0]):   # replays with other images: each equals the direct calls
                feed(pair)
                c.graph_launch(gid)
                assert snapshot() == direct[pair], pair
            c.graph_destroy(gid)
    finally:
        c.set_stream(None)
        c.close()


# ---- arguments -----------------------------------------------------------------------------------------------------------
def test_arguments_are_checked_on_a_live_context(images):
    img = images["97x80 texture"]
    c = capi.Context(0)
    try:
        c.frame_upload(2, img, 1)
        ok = capi.orb_params_default()
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=DEV)
        d_k, d_n, d_a, d_d, d_i = z((16, 2), torch.float32), z(1, torch.int32), z(16, torch.float32), z((17, 32), torch.uint8), z(8, torch.int32)
        with pytest.raises(capi.PagkError) as e:                     # no pattern yet
            c.orb_describe_device(ok, 2, 16, d_k, d_n, d_a, d_d, d_i)
        assert e.value.code == capi.PAGK_E_ARG and "pattern" in str(e.value)
        for pos, v in ((0, 14), (1023, -14)):
            pat = ou.seeded_pattern()
            pat[pos] = v
            with pytest.raises(capi.PagkError) as e:
                c.orb_set_pattern(pat)
            assert e.value.code == capi.PAGK_E_ARG
        with pytest.raises(capi.PagkError):                          # a refused pattern is not a pattern
            c.orb_describe_device(ok, 2, 16, d_k, d_n, d_a, d_d, d_i)
        c.orb_set_pattern(ou.seeded_pattern())
        c.orb_describe_device(ok, 2, 16, d_k, d_n, d_a, d_d, d_i)
        c.sync()
        for bad in (dict(blur_weights=(55, 49, 34, 18)), dict(blur_weights=(258, -1, 0, 0)), dict(n_levels=2)):
            with pytest.raises(capi.PagkError) as e:
                c.orb_describe_device(capi.orb_params_default(**bad), 2, 16, d_k, d_n, d_a, d_d, d_i)
            assert e.value.code == (capi.PAGK_E_UNSUPPORTED if "n_levels" in bad else capi.PAGK_E_ARG), bad
        for args in ((3, 16, d_k, d_n, d_a, d_d, d_i),                               # an empty slot
                     (2, 0, d_k, d_n, d_a, d_d, d_i), (2, (1 << 20) + 1, d_k, d_n, d_a, d_d, d_i),
                     (2, 16, d_k, d_n, d_a, d_d.view(-1)[8:], d_i)):                  # descriptors off the 16-byte boundary
            with pytest.raises(capi.PagkError):
                c.orb_describe_device(ok, *args)
        d_idx, d_dist, d_keep = z(16, torch.int32), z(16, torch.int32), z(16, torch.uint8)
        c.orb_match_device(ok, 16, d_d, d_n, 16, d_d, d_n, d_idx, d_dist, d_keep, d_i)
        c.sync()
        for args in ((0, d_d, d_n, 16, d_d, d_n), (16, d_d, d_n, 0, d_d, d_n), (16, d_d.view(-1)[8:], d_n, 16, d_d, d_n),
                     (16, d_d, d_n, (1 << 20) + 1, d_d, d_n), (16, d_d, None, 16, d_d, d_n)):
            with pytest.raises(capi.PagkError):
                c.orb_match_device(ok, *args, d_idx, d_dist, d_keep, d_i)
        with pytest.raises(capi.PagkError) as e:
            c.orb_match_device(capi.orb_params_default(match_floor=-1), 16, d_d, d_n, 16, d_d, d_n, d_idx, d_dist, d_keep, d_i)
        assert e.value.code == capi.PAGK_E_ARG
    finally:
        c.close()
