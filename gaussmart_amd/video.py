"""Trajectory videos: a Motion-JPEG AVI writer on PIL alone, the reference's create_videos (utils/render_utils.py:203-268) on
the files of an export, and export_trajectory, which goes from the maps in device memory to the same files and videos
without reading a file back.

    ex.reconstruction(generate_path(scene.getTrainCameras(), n_frames=240))
    export_trajectory(ex, traj_dir, "render_traj")          # renders/*.png, vis/depth_*.tiff, render_traj_{color,depth}.avi
"""
import io
import os
import struct

import numpy as np


class MJPEGWriter:
    """A RIFF `AVI ` file with one `vids` / `MJPG` stream: every frame is PIL's JPEG encoding of an u8 [H,W,3] (or [H,W])
    array in a `00dc` chunk, followed by an `idx1` index.  shape = (height, width), as mediapy's VideoWriter takes it.

        with MJPEGWriter(path, (H, W), fps=60) as w:
            w.add_image(frame)
    """
    _HEADER_BYTES = 12 + (12 + (8 + 56) + (12 + (8 + 56) + (8 + 40))) + 12     # RIFF, hdrl (avih, strl (strh, strf)), movi

    def __init__(self, path, shape, fps=60, quality=95):
        self.path, self.fps, self.quality = path, int(fps), int(quality)
        self.height, self.width = int(shape[0]), int(shape[1])
        self._index = []      # (offset from the `movi` fourcc, size) per frame
        self._max_chunk = 0
        self._f = open(path, "wb")
        self._f.write(b"\0" * self._HEADER_BYTES)
        self._movi_bytes = 4  # the `movi` fourcc itself

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def num_frames(self):
        return len(self._index)

    def encode(self, frame):
        """PIL's JPEG bytes of one frame at this writer's quality."""
        from PIL import Image
        frame = np.ascontiguousarray(frame, np.uint8)
        if frame.shape[:2] != (self.height, self.width):
            raise ValueError(f"MJPEGWriter: frame is {frame.shape[:2]}, the video {(self.height, self.width)}")
        buf = io.BytesIO()
        Image.fromarray(frame).save(buf, "JPEG", quality=self.quality)
        return buf.getvalue()

    def add_image(self, frame):
        self.add_jpeg(self.encode(frame))

    def add_jpeg(self, data):
        self._index.append((self._movi_bytes, len(data)))
        self._max_chunk = max(self._max_chunk, len(data))
        self._f.write(b"00dc" + struct.pack("<I", len(data)) + data + (b"\0" if len(data) % 2 else b""))
        self._movi_bytes += 8 + len(data) + len(data) % 2

    def close(self):
        if self._f is None:
            return
        f, n, w, h = self._f, len(self._index), self.width, self.height
        idx = b"".join(b"00dc" + struct.pack("<III", 0x10, off, size) for off, size in self._index)
        f.write(b"idx1" + struct.pack("<I", len(idx)) + idx)
        total = f.tell()
        avih = struct.pack("<14I", 1000000 // max(self.fps, 1), self._max_chunk * self.fps, 0, 0x10, n, 0, 1, self._max_chunk,
                           w, h, 0, 0, 0, 0)
        strh = b"vidsMJPG" + struct.pack("<IHHIIIIIIII4H", 0, 0, 0, 0, 1, self.fps, 0, n, self._max_chunk, 0xFFFFFFFF, 0,
                                         0, 0, w, h)
        strf = struct.pack("<IiiHH4sIiiII", 40, w, h, 1, 24, b"MJPG", w * h * 3, 0, 0, 0, 0)
        strl = b"strl" + b"strh" + struct.pack("<I", len(strh)) + strh + b"strf" + struct.pack("<I", len(strf)) + strf
        hdrl = b"hdrl" + b"avih" + struct.pack("<I", len(avih)) + avih + b"LIST" + struct.pack("<I", len(strl)) + strl
        head = (b"RIFF" + struct.pack("<I", total - 8) + b"AVI " + b"LIST" + struct.pack("<I", len(hdrl)) + hdrl +
                b"LIST" + struct.pack("<I", self._movi_bytes) + b"movi")
        assert len(head) == self._HEADER_BYTES
        f.seek(0)
        f.write(head)
        f.close()
        self._f = None


def load_img(pth):
    from PIL import Image
    with open(pth, 'rb') as f:
        return np.array(Image.open(f), dtype=np.float32)


def _open_writer(base_dir, video_prefix, k, shape, input_format):
    """(writer, path): the reference's mp4 through mediapy where it imports (its arguments: h264, 60 fps, crf 18), else a
    Motion-JPEG AVI at 60 fps."""
    try:
        import mediapy as media
    except ImportError:
        path = os.path.join(base_dir, f'{video_prefix}_{k}.avi')
        return MJPEGWriter(path, shape, fps=60), path
    path = os.path.join(base_dir, f'{video_prefix}_{k}.mp4')
    return media.VideoWriter(path, shape=shape, codec='h264', fps=60, crf=18, input_format=input_format), path


def create_videos(base_dir, input_dir, out_name, num_frames=480):
    """utils/render_utils.py:203-268 on the files of an export (input_dir/renders/*.png, input_dir/vis/depth_*.tiff): the
    depth limits are the log of the 3 % / 97 % depth of vis/depth_00000.tiff, a depth frame is turbo of the clipped log
    depth, a tag without files is skipped.  Writes base_dir/<out_name>_{depth,color}.avi (.mp4 where mediapy imports)."""
    from .frames import depth_limits_host, depth_to_turbo_host
    video_prefix = f'{out_name}'
    zpad = max(5, len(str(num_frames - 1)))

    def idx_to_str(idx):
        return str(idx).zfill(zpad)

    os.makedirs(base_dir, exist_ok=True)
    depth_frame = load_img(os.path.join(input_dir, 'vis', f'depth_{idx_to_str(0)}.tiff'))
    shape = depth_frame.shape
    lo, hi = depth_limits_host(depth_frame, p=3)
    print(f'Video shape is {shape[:2]}')
    for k in ['depth', 'normal', 'color']:
        file_ext = 'png' if k in ['color', 'normal'] else 'tiff'

        def img_file(idx):
            if k == 'color':
                return os.path.join(input_dir, 'renders', f'{idx_to_str(idx)}.{file_ext}')
            return os.path.join(input_dir, 'vis', f'{k}_{idx_to_str(idx)}.{file_ext}')

        if not os.path.exists(img_file(0)):
            print(f'Images missing for tag {k}')
            continue
        writer, video_file = _open_writer(base_dir, video_prefix, k, shape[:2], 'gray' if k == 'alpha' else 'rgb')
        print(f'Making video {video_file}...')
        with writer:
            for idx in range(num_frames):
                img = load_img(img_file(idx))
                if k in ['color', 'normal']:
                    img = img / 255.
                    frame = (np.clip(np.nan_to_num(img), 0., 1.) * 255.).astype(np.uint8)
                else:
                    frame = depth_to_turbo_host(img, lo, hi)[1]
                writer.add_image(frame)


def export_trajectory(extractor, traj_dir, out_name, host=False):
    """The frames and videos of extractor's views (GaussianExtractor.reconstruction over a camera path): renders/NNNNN.png,
    vis/depth_NNNNN.tiff and <out_name>_{color,depth}.avi under traj_dir.

    Default: the device route.  Colours become u8 and depth becomes the cleaned fp32 map and its turbo frame in kernels
    (gaussmart_amd/frames.py); only those cross to the host, where each is encoded once for its file and once for its
    video.  The depth limits come from frame 0's depth (one sort, four floats read back).  No file is read back.
    host=True: export_image(host=True), then create_videos over the files it wrote."""
    n = len(extractor.viewpoint_stack)
    if host:
        extractor.export_image(traj_dir, host=True)
        create_videos(base_dir=traj_dir, input_dir=traj_dir, out_name=out_name, num_frames=n)
        return
    from PIL import Image
    from .frames import depth_limits, depth_to_turbo, to_u8
    render_path, vis_path = os.path.join(traj_dir, "renders"), os.path.join(traj_dir, "vis")
    for d in (render_path, vis_path, os.path.join(traj_dir, "gt")):
        os.makedirs(d, exist_ok=True)
    if n == 0:
        return
    lo, hi = depth_limits(extractor.depthmaps[0], p=3)
    H, W = extractor.depthmaps[0].shape[-2:]
    print(f'Video shape is {(H, W)}')
    color_writer, color_file = _open_writer(traj_dir, out_name, 'color', (H, W), 'rgb')
    depth_writer, depth_file = _open_writer(traj_dir, out_name, 'depth', (H, W), 'rgb')
    print(f'Making video {depth_file}...')
    print(f'Making video {color_file}...')
    with color_writer, depth_writer:
        for idx, cam in enumerate(extractor.viewpoint_stack):
            if getattr(cam, "original_image", None) is not None:
                Image.fromarray(to_u8(cam.original_image[0:3].to(extractor.rgbmaps[idx].device)).cpu().numpy()).save(
                    os.path.join(traj_dir, "gt", f"{idx:05d}.png"), "PNG")
            rgb = to_u8(extractor.rgbmaps[idx]).cpu().numpy()
            clean, turbo = depth_to_turbo(extractor.depthmaps[idx], lo, hi)
            Image.fromarray(rgb).save(os.path.join(render_path, f"{idx:05d}.png"), "PNG")
            Image.fromarray(clean.reshape(H, W).cpu().numpy()).save(os.path.join(vis_path, f"depth_{idx:05d}.tiff"), "TIFF")
            color_writer.add_image(rgb)
            depth_writer.add_image(turbo.cpu().numpy())
