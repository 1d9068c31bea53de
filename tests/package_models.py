"""What the two test files of the opened viewer package share (tests/test_open_package_cpu.py, tests/test_gpu_open_package.py): the fp64
statement of "target pixel -> lattice coordinate" of a camera and a spec, and the poses of the render tests."""
import numpy as np
import torch


def lattice_coords(camera, spec, extrins, intrins, H, W, planes=None):
    """fp64: pixel (x, y) of an H x W view -> the coordinate the render samples plane d at, [N,D,H,W,2] (x, y): `camera.plane_homographies`
    (the module's own code object; its float32 matrices) applied to the pixel centre, then spec.scale / spec.offset.  extrins [N,4,4]
    world-to-camera, intrins [N,3,3]; planes: the planes to keep (default all)."""
    extrins, intrins = torch.as_tensor(extrins, dtype=torch.float32), torch.as_tensor(intrins, dtype=torch.float32)
    ref_inv = camera._on(extrins.device, "ref_extrin")[None].inverse().to(extrins.dtype)
    ys, xs = np.meshgrid(np.arange(H) + spec.pixel_center, np.arange(W) + spec.pixel_center, indexing="ij")
    p = np.stack([xs, ys, np.ones_like(xs)], 0).reshape(3, -1)                                  # 3,HW
    out = []
    for i in range(len(extrins)):
        h = camera.plane_homographies(extrins[i:i + 1] @ ref_inv, intrins[i:i + 1]).double().numpy()      # D,3,3
        if planes is not None:
            h = h[planes]
        q = h @ p                                                                               # D,3,HW
        xy = np.stack([q[:, 0] / q[:, 2] * spec.scale[0] + spec.offset[0], q[:, 1] / q[:, 2] * spec.scale[1] + spec.offset[1]], -1)
        out.append(xy.reshape(len(h), H, W, 2))
    return np.stack(out)


def border_distance(coords, tile):
    """smallest distance of any coordinate of `coords` [...,2] to a tile border (a multiple of tw - 1 in x, of th - 1 in y; the plane's edges
    are two of them)."""
    sx, sy = tile[1] - 1, tile[0] - 1
    dx = np.abs(coords[..., 0] - np.rint(coords[..., 0] / sx) * sx)
    dy = np.abs(coords[..., 1] - np.rint(coords[..., 1] / sy) * sy)
    return float(min(dx.min(), dy.min()))


def tilted_pose(i, attempt=0):
    """world-to-camera pose i of the render tests: a rotation about all three axes and a translation, both a little different for every
    `attempt` (moving a pose off a tile border)."""
    a = 0.01 * (i + 1) + 0.00137 * attempt
    rx, ry, rz = 0.7 * a, -a, 0.5 * a
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    R = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    e = np.eye(4, dtype=np.float32)
    e[:3, :3] = R
    e[:3, 3] = [0.031 * np.cos(1.3 * i) + 0.0011 * attempt, 0.023 * np.sin(0.9 * i + 0.4), 0.011 * np.sin(2.1 * i)]
    return e


def clear_poses(camera, spec, K, H, W, n, margin=1e-3, tries=400):
    """n tilted poses under which, in fp64, no sample coordinate of any pixel on any plane lies within `margin` lattice units of a tile border
    or a plane edge: pose i is tilted_pose(i, attempt) of the first attempt that is clear (a pose on a border is moved).  -> extrins [n,4,4]."""
    out = []
    for i in range(n):
        for attempt in range(tries):
            e = tilted_pose(i, attempt)
            if border_distance(lattice_coords(camera, spec, e[None], K[None], H, W), spec.tile) > margin:
                out.append(e)
                break
        else:
            raise AssertionError(f"pose {i}: no attempt of {tries} keeps every sample {margin} away from the tile borders")
    return np.stack(out)
