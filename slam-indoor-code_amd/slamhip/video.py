"""Motion-JPEG video: cv::VideoCapture(path, CAP_OPENCV_MJPEG) over the AVI walker
(slam_avi_index) and the JPEG decoder, a minimal AVI writer for already-encoded
streams, and cv::VideoWriter over the JPEG encoder.  The reference reads every frame through VideoCapture::read
(mainCycleInternals.cpp:107-119); inter-frame codecs are out of scope, and any video
becomes Motion-JPEG with one transcode."""
import mmap
import os
import struct

import numpy as np

from . import _lib as L
from . import api

CAP_PROP_POS_FRAMES = 1
CAP_PROP_FRAME_WIDTH = 3
CAP_PROP_FRAME_HEIGHT = 4
CAP_PROP_FPS = 5
CAP_PROP_FRAME_COUNT = 7


class VideoCapture:
    """cv::VideoCapture over a Motion-JPEG AVI file (a path, mapped read-only) or its
    bytes.  read() decodes one frame (on the device with a context, else with the
    host decoder); read_batch(n) decodes the next n frames in one
    slam_jpeg_decode_batch_dev_ex call straight from the mapped file into a resident
    (n, h, w, 3) tensor.  Frames are parsed with L.JPEG_MJPEG (streams without DHT
    take the Annex K tables); the Exif orientation is ignored, as that backend
    ignores it.  A file the walker refuses leaves the capture closed (isOpened()
    False, `error` holds the SlamError), as cv::VideoCapture::open returns false."""

    def __init__(self, path_or_bytes, ctx=None):
        self.ctx = ctx
        self.error = None
        self._file = self._map = None
        self._buf = None
        self._pos = 0
        self.info, self._off, self._size = None, None, None
        try:
            if isinstance(path_or_bytes, (str, os.PathLike)):
                self._file = open(path_or_bytes, "rb")
                self._map = mmap.mmap(self._file.fileno(), 0, access=mmap.ACCESS_READ)
                self._buf = np.frombuffer(self._map, np.uint8)
            else:
                self._buf = np.frombuffer(path_or_bytes, np.uint8)
            self.info, self._off, self._size = api.aviIndex(self._buf)
        except (OSError, ValueError, L.SlamError) as e:
            self.error = e
            self.release()

    def isOpened(self):
        return self.info is not None

    def release(self):
        self.info = self._off = self._size = None
        self._buf = None
        if self._map is not None:
            try:
                self._map.close()
            except BufferError:      # a frame view still alive keeps the mapping; it goes with the view
                pass
            self._map = None
        if self._file is not None:
            self._file.close()
            self._file = None

    def get(self, prop):
        if not self.isOpened():
            return 0.0
        if prop == CAP_PROP_FRAME_COUNT:
            return float(self.info["frames"])
        if prop == CAP_PROP_FPS:
            return float(self.info["fps"])
        if prop == CAP_PROP_FRAME_WIDTH:
            return float(self.info["width"])
        if prop == CAP_PROP_FRAME_HEIGHT:
            return float(self.info["height"])
        if prop == CAP_PROP_POS_FRAMES:
            return float(self._pos)
        return 0.0

    def set(self, prop, value):
        """CAP_PROP_POS_FRAMES only: every frame is a key frame, so the seek is exact"""
        if not self.isOpened() or prop != CAP_PROP_POS_FRAMES:
            return False
        v = int(value)
        if v < 0 or v > self.info["frames"]:
            return False
        self._pos = v
        return True

    def stream(self, i):
        """the JPEG stream of frame i (a view of the file)"""
        o, n = int(self._off[i]), int(self._size[i])
        return self._buf[o:o + n]

    def read(self):
        """(ok, BGR frame): (False, None) at the end of the stream or for a frame that cannot be decoded"""
        if not self.isOpened() or self._pos >= self.info["frames"]:
            return False, None
        data = self.stream(self._pos)
        self._pos += 1
        try:
            if self.ctx is None:
                frame, _ = api.imdecode_host(data, L.JPEG_MJPEG)
            else:
                dev, status, _ = api.imdecode_batch([data], ctx=self.ctx, parallel=True, flags=L.JPEG_MJPEG)
                if status[0] < 0:
                    return False, None
                frame = dev[0].cpu().numpy()
        except L.SlamError:
            return False, None
        return True, frame

    def read_batch(self, n, out=None):
        """the next min(n, frames left) frames as a resident (k, h, w, 3) tensor, and
        their status words (imdecode_batch's); (None, None) at the end of the stream"""
        if not self.isOpened():
            return None, None
        k = min(int(n), self.info["frames"] - self._pos)
        if k <= 0:
            return None, None
        ctx = self.ctx or api.default_context()
        bufs = [self.stream(self._pos + i) for i in range(k)]
        dev, status, _ = api.imdecode_batch(bufs, ctx=ctx, out=out, size=(self.info["width"], self.info["height"]),
                                            parallel=True, flags=L.JPEG_MJPEG)
        self._pos += k
        return dev, status


def write_mjpeg_avi(path, jpeg_streams, fps, size):
    """A minimal Motion-JPEG AVI: hdrl (avih, one strl with strh and strf), one movi
    of 00dc chunks and idx1.  jpeg_streams: the frames, already encoded (VideoWriter
    below encodes them); fps: a number or (rate, scale); size: (width, height).  Returns
    the number of bytes written."""
    streams = [bytes(s) for s in jpeg_streams]
    w, h = int(size[0]), int(size[1])
    rate, scale = (int(fps[0]), int(fps[1])) if isinstance(fps, (tuple, list)) else (int(round(float(fps) * 1000)), 1000)
    n = len(streams)
    biggest = max([len(s) for s in streams] + [0])

    def chunk(cc, data):
        return cc + struct.pack("<I", len(data)) + data + (b"\0" if len(data) & 1 else b"")

    def lst(kind, data):
        return b"LIST" + struct.pack("<I", 4 + len(data)) + kind + data

    avih = struct.pack("<14I", int(1e6 * scale / rate) if rate else 0, 0, 0, 0x10, n, 0, 1, biggest, w, h, 0, 0, 0, 0)
    strh = struct.pack("<4s4sIHHIIIIIIII4H", b"vids", b"MJPG", 0, 0, 0, 0, scale, rate, 0, n, biggest, 0xFFFFFFFF, 0,
                       0, 0, w, h)
    strf = struct.pack("<IiiHH4sIiiII", 40, w, h, 1, 24, b"MJPG", w * h * 3, 0, 0, 0, 0)
    hdrl = lst(b"hdrl", chunk(b"avih", avih) + lst(b"strl", chunk(b"strh", strh) + chunk(b"strf", strf)))
    body, index, off = [], [], 4
    for s in streams:
        c = chunk(b"00dc", s)
        index.append(struct.pack("<4sIII", b"00dc", 0x10, off, len(s)))
        body.append(c)
        off += len(c)
    movi = lst(b"movi", b"".join(body))
    idx1 = chunk(b"idx1", b"".join(index))
    riff = b"AVI " + hdrl + movi + idx1
    data = b"RIFF" + struct.pack("<I", len(riff)) + riff
    with open(path, "wb") as f:
        f.write(data)
    return len(data)


class VideoWriter:
    """cv::VideoWriter(path, fourcc "MJPG", fps, size) over the device JPEG encoder:
    write(frame) and write_batch(frames) encode (h, w, 3) BGR frames (numpy, or
    resident torch tensors) with api.imencode_batch, the streams are buffered, and
    release() writes the file through write_mjpeg_avi.  size: (width, height);
    restart_rows: a restart interval of that many MCU rows (0: none), which is what
    the decoder reads fastest.  Deviation: OpenCV's built-in Motion-JPEG writer is an
    encoder of its own with other arithmetic and its own default quality; this one
    writes imencode's frames (libjpeg's bytes).  host=True encodes numpy frames with
    the host encoder instead (the same bytes, no GPU).  A fourcc other than MJPG, or a
    size that is not positive, leaves the writer closed (isOpened() False)."""

    def __init__(self, path, fourcc="MJPG", fps=30.0, size=None, quality=95, sampling=L.JPEG_420, restart_rows=0, ctx=None, host=False):
        self.path, self.fps, self.ctx, self.host = path, fps, ctx, bool(host)
        self.quality, self.sampling, self.restart_rows = int(quality), int(sampling), int(restart_rows)
        self.size = (int(size[0]), int(size[1])) if size is not None else None
        self.streams = []
        name = fourcc.decode() if isinstance(fourcc, bytes) else str(fourcc)
        self._open = name.upper() == "MJPG" and self.size is not None and min(self.size) > 0 and self.restart_rows >= 0
        self.bytes_written = 0

    def isOpened(self):
        return self._open

    def _restart(self):
        hs = 1 if self.sampling in (L.JPEG_GRAY, L.JPEG_444) else 2
        return min(self.restart_rows * ((self.size[0] + 8 * hs - 1) // (8 * hs)), 65535)

    def write_batch(self, frames):
        """encodes (n, h, w, 3) frames in one set of launches and buffers their streams"""
        if not self._open:
            raise ValueError("VideoWriter is not open")
        shape = tuple(int(v) for v in frames.shape)
        if len(shape) != 4 or shape[1:] != (self.size[1], self.size[0], 3):
            raise ValueError(f"frames are (n, {self.size[1]}, {self.size[0]}, 3) uint8")
        if shape[0] and self.host:
            for f in np.asarray(frames):
                self.streams.append(api.jpegEncode(f, self.quality, self.sampling, self._restart(), host=True)[0])
        elif shape[0]:
            self.streams += api.imencode_batch(frames, self.quality, self.sampling, self._restart(), ctx=self.ctx)

    def write(self, frame):
        self.write_batch(frame[None])

    def release(self):
        """writes the file (once); returns the bytes written"""
        if self._open:
            self._open = False
            self.bytes_written = write_mjpeg_avi(self.path, self.streams, self.fps, self.size)
            self.streams = []
        return self.bytes_written
