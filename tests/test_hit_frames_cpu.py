"""CPU checks of the frames-of-a-hit entry: its C-ABI signature as hmmc_amd/_lib.py derives it from include/hmmc_hip.h
(tests/test_abi.py holds header, exports and ctypes together), the numpy restatement tests/hit_frames_ref.py against the
reference's golden (tests/golden/head_eval.npz: the mean of the k best frame logits is the reference's top-k term, the video
logit its S_video), and the restatement's own conventions on hand-written data."""
import numpy as np

import hit_frames_ref as R
from conftest import golden
from hmmc_amd import _lib, synth


def test_hit_frames_signature_follows_the_header():
    # const float* x 2, const int* x 2, float*, int*, float*, long, int x 6, float, hmmc_stream_t -> int
    assert _lib.SIGNATURES["hmmc_hit_frames"] == ("pppppppliiiiiifp", "i")
    from hmmc_amd import ops
    assert callable(ops.hit_frames)


def test_reference_reproduces_the_golden_topk_terms():
    g = golden("head_eval")
    q = synth.normal("head_eval.q", (48, 512)).double().numpy()
    v = synth.normal("head_eval.v", (48, 512)).double().numpy()
    u = synth.normal("head_eval.u", (48, 12, 512)).double().numpy()
    q = q + 0.7 * v
    q /= np.linalg.norm(q, axis=-1, keepdims=True)
    packed = R.pack(v, u)
    pq, pv = [a.ravel() for a in np.meshgrid(np.arange(48), np.arange(48), indexing="ij")]
    ks = sorted(int(name[4:]) for name in g.files if name.startswith("topk"))
    assert ks == [1, 2, 3, 12]
    for k in ks:
        fs, fi, vl = R.hit_frames(q, packed, pq, pv, 48, 12, k, 100.0)
        assert fs.shape == (48 * 48, k) and fi.min() >= 0 and fi.max() < 12
        err = np.abs(fs.mean(-1).reshape(48, 48) - g[f"topk{k}"]).max()
        assert err < 1e-3, (k, err)
        err = np.abs(vl.reshape(48, 48) - g["S_video"]).max()
        assert err < 1e-3, err
        assert all(len(set(row)) == k for row in fi.tolist())


def test_reference_conventions():
    E, F, k = 4, 3, 3
    q = np.array([[1, 0, 0, 0], [-1, 0, 0, 0]], np.float32)
    packed = np.zeros((2 * 16, E), np.float32)
    packed[0, 0] = 2                                    # video 0: slot 0
    packed[1:4, 0] = [1, 2, 1]                          # frames 0 and 2 tie
    packed[16 + 1, 0] = np.nan                          # video 1: frame 0 NaN, frame 1 zero, frame 2 negative
    packed[16 + 3, 0] = -1
    pq = np.array([0, 0, 1, 5, 0, -1])
    pv = np.array([7, 8, 7, 7, 9, 7])                   # chunk = videos 7, 8
    fs0 = np.full((6, k), 42, np.float32)
    fs, fi, vl = R.hit_frames(q, packed, pq, pv, 2, F, k, 0.5, video_base=7, frame_score=fs0, dtype=np.float32)
    assert fs.dtype == np.float32 and fi.dtype == np.int32
    assert fs[0].tolist() == [1.0, 0.5, 0.5] and fi[0].tolist() == [1, 0, 2] and vl[0] == 1.0
    assert fs[1].tolist() == [0.0, -0.5, -np.inf] and fi[1].tolist() == [1, 2, 0]
    # query 1 = -query 0: frame 1 of video 7 leads now; on video 8 the zero frame's logit is -0 and must come back as +0
    assert fs[2].tolist() == [-0.5, -0.5, -1.0] and fi[2].tolist() == [0, 2, 1]
    fs2, fi2, _ = R.hit_frames(q, packed, [1], [8], 2, F, k, 0.5, video_base=7, dtype=np.float32)
    assert fs2[0].tolist() == [0.5, 0.0, -np.inf] and fi2[0].tolist() == [2, 1, 0] and not np.signbit(fs2[0, 1])
    for m in (3, 4, 5):                                 # query 5, video 9, query -1: untouched
        assert fs[m].tolist() == [42, 42, 42] and fi[m].tolist() == [-1, -1, -1] and np.isnan(vl[m])
