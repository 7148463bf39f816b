"""The fly-around camera path of the reference's utils/render_utils.py (normalize .. generate_path, lines 28-66 and 76-194):
the training poses are rotated onto their principal axes, an ellipse is laid through them at height 0, and every position
looks at the point nearest to all focal axes.  Host code, numpy in float64, the same calls in the same order as the
reference, so the poses agree with it to rounding.

    from gaussmart_amd.render_path import generate_path
    traj = generate_path(scene.getTrainCameras(), n_frames=240)
    extractor.reconstruction(traj)
"""
import copy

import numpy as np
import torch

from .mesh import focus_point_fn


def normalize(x):
    return x / np.linalg.norm(x)


def pad_poses(p):
    """[..., 3, 4] poses with the homogeneous bottom row [0, 0, 0, 1]."""
    bottom = np.broadcast_to([0, 0, 0, 1.], p[..., :1, :4].shape)
    return np.concatenate([p[..., :3, :4], bottom], axis=-2)


def unpad_poses(p):
    return p[..., :3, :4]


def viewmatrix(lookdir, up, position):
    """Look-at camera-to-world matrix [3,4]: columns x, y, z, position."""
    vec2 = normalize(lookdir)
    vec0 = normalize(np.cross(up, vec2))
    vec1 = normalize(np.cross(vec2, vec0))
    return np.stack([vec0, vec1, vec2, position], axis=1)


def transform_poses_pca(poses):
    """(poses_recentered [N,3,4], transform [4,4]): the camera-to-world poses [N,3,4] with their positions' principal
    components on the x, y, z axes (largest first), a proper rotation, and the mean y-axis pointing up (z > 0)."""
    t = poses[:, :3, 3]
    t_mean = t.mean(axis=0)
    t = t - t_mean
    eigval, eigvec = np.linalg.eig(t.T @ t)
    inds = np.argsort(eigval)[::-1]
    eigvec = eigvec[:, inds]
    rot = eigvec.T
    if np.linalg.det(rot) < 0:
        rot = np.diag(np.array([1, 1, -1])) @ rot
    transform = np.concatenate([rot, rot @ -t_mean[:, None]], -1)
    poses_recentered = unpad_poses(transform @ pad_poses(poses))
    transform = np.concatenate([transform, np.eye(4)[3:]], axis=0)
    if poses_recentered.mean(axis=0)[2, 1] < 0:
        poses_recentered = np.diag(np.array([1, -1, -1])) @ poses_recentered
        transform = np.diag(np.array([1, -1, -1, 1])) @ transform
    return poses_recentered, transform


def generate_ellipse_path(poses, n_frames=120, const_speed=True, z_variation=0., z_phase=0.):
    """[n_frames,3,4] poses on an ellipse around the focus point of `poses`, its axes the 90th percentile of the camera
    offsets.  const_speed is accepted and ignored, as in the reference (its resampling is commented out)."""
    center = focus_point_fn(poses)
    offset = np.array([center[0], center[1], 0])
    sc = np.percentile(np.abs(poses[:, :3, 3] - offset), 90, axis=0)
    low = -sc + offset
    high = sc + offset
    z_low = np.percentile((poses[:, :3, 3]), 10, axis=0)
    z_high = np.percentile((poses[:, :3, 3]), 90, axis=0)

    def get_positions(theta):
        return np.stack([
            low[0] + (high - low)[0] * (np.cos(theta) * .5 + .5),
            low[1] + (high - low)[1] * (np.sin(theta) * .5 + .5),
            z_variation * (z_low[2] + (z_high - z_low)[2] * (np.cos(theta + 2 * np.pi * z_phase) * .5 + .5)),
        ], -1)

    theta = np.linspace(0, 2. * np.pi, n_frames + 1, endpoint=True)
    positions = get_positions(theta)[:-1]
    avg_up = poses[:, :3, 1].mean(0)
    avg_up = avg_up / np.linalg.norm(avg_up)
    ind_up = np.argmax(np.abs(avg_up))
    up = np.eye(3)[ind_up] * np.sign(avg_up[ind_up])
    return np.stack([viewmatrix(p - center, up, p) for p in positions])


def path_c2ws(c2ws, n_frames):
    """[n_frames,4,4] camera-to-world matrices (the renderer's axes) of the path through the cameras c2ws [N,4,4]."""
    flip = np.diag([1, -1, -1, 1])
    pose = c2ws[:, :3, :] @ flip
    pose_recenter, colmap_to_world_transform = transform_poses_pca(pose)
    new_poses = generate_ellipse_path(poses=pose_recenter, n_frames=n_frames)
    new_poses = np.linalg.inv(colmap_to_world_transform) @ pad_poses(new_poses)
    return new_poses @ flip


def generate_path(viewpoint_cameras, n_frames=480, device=None):
    """Cameras render() accepts along the ellipse through viewpoint_cameras.  Each is a shallow copy of camera 0 with
    image_height / image_width rounded down to even, world_view_transform = inv(c2w).T as float32, full_proj_transform and
    camera_center derived from it, on `device` (default: camera 0's).

    DEVIATION: original_image and gt_alpha_mask are None.  The reference deep-copies camera 0, photograph included, so its
    export writes camera 0's picture once per frame into traj/.../gt; these cameras carry no picture and no gt is written."""
    cam0 = viewpoint_cameras[0]
    dev = cam0.world_view_transform.device if device is None else torch.device(device)
    c2ws = np.array([np.linalg.inv(np.asarray(cam.world_view_transform.T.cpu().numpy())) for cam in viewpoint_cameras])
    proj = cam0.projection_matrix.to(dev)
    traj = []
    for c2w in path_c2ws(c2ws, n_frames):
        cam = copy.copy(cam0)
        cam.image_height = int(cam0.image_height / 2) * 2
        cam.image_width = int(cam0.image_width / 2) * 2
        cam.world_view_transform = torch.from_numpy(np.linalg.inv(c2w).T).float().to(dev)
        cam.full_proj_transform = cam.world_view_transform @ proj
        cam.camera_center = cam.world_view_transform.inverse()[3, :3].contiguous()
        cam.original_image = None
        cam.gt_alpha_mask = None
        traj.append(cam)
    return traj
