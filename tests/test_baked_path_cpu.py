"""How render_frames(baked=) launches a selection (videoloop3d_amd/render_video.path_segments): a chunk that is exactly one run -- one camera,
consecutive frames of the clip -- keeps the frame-pair call, every other chunk is one path call (render.render_path_baked).  Pure: no device."""
import numpy as np

from videoloop3d_amd import render_video as RV


def _selection(v="", t="", T=5, n=12):
    """(cam_of, render_t) of script_render_video.py's selection on n spiral poses and 4 training views, cameras numbered by first appearance
    as baked.path_cameras numbers them."""
    rp = np.arange(n * 12, dtype=np.float32).reshape(n, 3, 4)
    ri = np.tile(np.eye(3, dtype=np.float32), (n, 1, 1))
    tp = -np.arange(4 * 12, dtype=np.float32).reshape(4, 3, 4) - 1
    ti = 2 * np.tile(np.eye(3, dtype=np.float32), (4, 1, 1))
    vp, vi, rt = RV.select_views_times(rp, ri, tp, ti, T, v=v, t=t)
    seen, cam_of = {}, []
    for p, k in zip(vp, vi):
        cam_of.append(seen.setdefault((p.tobytes(), k.tobytes()), len(seen)))
    return cam_of, rt[:len(cam_of)]


def test_a_spiral_is_one_path_segment_per_chunk():
    cam_of, rt = _selection()
    assert cam_of == list(range(12)) and rt.tolist() == [0, 1, 2, 3, 4, 0, 1, 2, 3, 4, 0, 1]
    assert RV.path_segments(cam_of, rt, 64) == [("path", 0, 12)]
    assert RV.path_segments(cam_of, rt, 12) == [("path", 0, 12)]
    assert RV.path_segments(cam_of, rt, 5) == [("path", 0, 5), ("path", 5, 10), ("path", 10, 12)]
    # a chunk of one frame is a run of one frame: nothing to gain from a path call
    assert RV.path_segments(cam_of, rt, 1) == [("run", i, i + 1) for i in range(12)]


def test_a_fixed_view_gives_runs():
    for v in ("r1", "2"):
        cam_of, rt = _selection(v=v)
        assert cam_of == [0] * 5 and rt.tolist() == [0, 1, 2, 3, 4]
        assert RV.path_segments(cam_of, rt, 64) == [("run", 0, 5)]
        assert RV.path_segments(cam_of, rt, 2) == [("run", 0, 2), ("run", 2, 4), ("run", 4, 5)]


def test_a_mixed_selection_splits_where_camera_or_frame_order_breaks():
    # one camera, the loop played twice: the frame order breaks at 4 -> 0.  Chunks that end at the break are runs; a chunk across it is a path
    cam_of, rt = [0] * 10, np.array([0, 1, 2, 3, 4, 0, 1, 2, 3, 4])
    assert RV.path_segments(cam_of, rt, 5) == [("run", 0, 5), ("run", 5, 10)]
    assert RV.path_segments(cam_of, rt, 64) == [("path", 0, 10)]
    assert RV.path_segments(cam_of, rt, 4) == [("run", 0, 4), ("path", 4, 8), ("run", 8, 10)]
    # a fixed view played backwards (--t 4:0) and a repeated frame: no run
    cam_of, rt = _selection(v="r1", t="4:0")
    assert rt.tolist() == [4, 3, 2, 1] and RV.path_segments(cam_of, rt, 64) == [("path", 0, 4)]
    assert RV.path_segments([0, 0, 0], [2, 2, 3], 64) == [("path", 0, 3)]
    # consecutive frames, the camera changes after the third: the break is inside the first chunk of 4, not inside the chunks of 3
    cam_of, rt = [0, 0, 0, 1, 1, 1], [0, 1, 2, 3, 4, 5]
    assert RV.path_segments(cam_of, rt, 4) == [("path", 0, 4), ("run", 4, 6)]
    assert RV.path_segments(cam_of, rt, 3) == [("run", 0, 3), ("run", 3, 6)]
    # a camera that comes back is still a break
    assert RV.path_segments([0, 1, 0], [0, 1, 2], 64) == [("path", 0, 3)]


def test_chunk_boundaries_are_respected():
    cam_of, rt = _selection(n=12)
    for chunk in (1, 2, 5, 7, 12, 13, 64):
        segs = RV.path_segments(cam_of, rt, chunk)
        assert segs[0][1] == 0 and segs[-1][2] == 12
        assert all(a[2] == b[1] for a, b in zip(segs, segs[1:]))                  # contiguous, in order
        assert all(0 < j - i <= max(1, chunk) for _, i, j in segs)                # never longer than a chunk
        assert all(j - i == min(chunk, 12) for _, i, j in segs[:-1])              # only the last one may be short
    assert RV.path_segments([], [], 64) == []
    assert RV.path_segments(cam_of, rt, 0) == RV.path_segments(cam_of, rt, 1)    # (render_frames clamps its max_batch the same way)
