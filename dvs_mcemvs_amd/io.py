"""On-disk formats at the edges of the DSI path, so that the
reference's own Python tools can consume this engine's outputs and its recorded
trajectories can be replayed without ROS:

  write_grid_npy        Grid3D::writeGridNpy           cartesian3dgrid_IO.cpp:30-36   (.npy, shape {Z,Y,X} f32)
  write_png_gray8       cv::imwrite of a CV_8UC1 slice  cartesian3dgrid_IO.cpp:74              (.png, 8-bit grayscale)
  write_png_rgb8        cv::imwrite of a CV_8UC3 image  utils.cpp:93                            (.png, 8-bit colour, from B G R)
  save_depth_points     saveDepthMaps (txt part)        utils.cpp:31-46                ("col row depth" lines)
  load_depth_points     its inverse, as scripts/evaluate_mcemvs_dsec.py:69-79 reads it (255 = no estimate)
  read_png_gray16       plt.imread of a DSEC disparity image, scripts/evaluate_mcemvs_dsec.py:99 (.png, 16-bit grayscale: the samples)
  write_png_gray16      test helper: the same format, with any of the five filter types
  dsec_disparity_name   the file name of a ground-truth frame, scripts/evaluate_mcemvs_dsec.py:99
  save_depth_maps       saveDepthMaps                  utils.cpp:22-104               (the txt and the two .png it writes)
  save_pcd_ascii        pcl::io::savePCDFileASCII       main.cpp:397-402               (.pcd v0.7, PointXYZI, ascii)
  save_pcd_normals_ascii, load_pcd_normals_ascii   the same for PointNormal (a world map's cells with WorldMap.fetchPca's normals)
  read_pose_bag         parse of geometry_msgs/PoseStamped bags   data_loading.cpp:221-302 (ROSBAG v2.0; none / bz2 chunks)
  read_event_bag        parse of dvs_msgs/EventArray bags         data_loading.cpp:31-107, 211-216
  write_pose_bag, write_event_bag   test helpers: minimal writers of the same subset of the format

Host-side file I/O only; nothing here touches voxels.  The .pcd layout is restated from PCL's documentation of the
format and is not pinned against a PCL build (none is available to this project).
"""
import bz2
import struct
import zlib

import numpy as np


def write_grid_npy(path, grid):
    """grid: engine Grid3D (downloaded here) or a numpy array [Z][Y][X]; float32 C order, like
    cnpy::npy_save(filename, &data_array_[0], {size_[2], size_[1], size_[0]}, "w")."""
    vol = grid.download() if hasattr(grid, "download") else np.asarray(grid)
    vol = np.ascontiguousarray(vol, np.float32)
    assert vol.ndim == 3
    with open(path, "wb") as f:
        np.save(f, vol, allow_pickle=False)
    return vol.shape


def _png_chunk(kind, body):
    return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body) & 0xffffffff)


def write_png_gray8(path, img):
    """An 8-bit grayscale PNG of a uint8 [rows][cols] image (Grid3D.imwriteSlices): IHDR, one IDAT holding the zlib
    stream of the scanlines, each with filter type 0, IEND.  Any PNG reader shows the pixels that were written; the
    bytes of the file are not those of OpenCV's encoder (other filters, other compression level)."""
    img = np.ascontiguousarray(img)
    if img.dtype != np.uint8 or img.ndim != 2 or img.shape[0] < 1 or img.shape[1] < 1:
        raise ValueError("write_png_gray8 takes a non-empty 2-D uint8 image")
    rows, cols = img.shape
    raw = np.zeros((rows, cols + 1), np.uint8)
    raw[:, 1:] = img

    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + _png_chunk(b"IHDR", struct.pack(">IIBBBBB", cols, rows, 8, 0, 0, 0, 0)) +
                _png_chunk(b"IDAT", zlib.compress(raw.tobytes(), 6)) + _png_chunk(b"IEND", b""))
    return rows, cols


def write_png_rgb8(path, img_bgr):
    """An 8-bit colour PNG (colour type 2) of a uint8 [rows][cols][3] image in OpenCV's channel order B G R, swapped to
    R G B on writing; scanlines with filter type 0, like write_png_gray8."""
    img = np.ascontiguousarray(img_bgr)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3 or img.shape[0] < 1 or img.shape[1] < 1:
        raise ValueError("write_png_rgb8 takes a non-empty uint8 image of shape (rows, cols, 3)")
    rows, cols = img.shape[:2]
    raw = np.zeros((rows, 3 * cols + 1), np.uint8)
    raw[:, 1:] = img[:, :, ::-1].reshape(rows, 3 * cols)
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + _png_chunk(b"IHDR", struct.pack(">IIBBBBB", cols, rows, 8, 2, 0, 0, 0)) +
                _png_chunk(b"IDAT", zlib.compress(raw.tobytes(), 6)) + _png_chunk(b"IEND", b""))
    return rows, cols


def write_png_gray16(path, img, filters=0):
    """A 16-bit grayscale PNG (colour type 0, samples big-endian) of a uint16 [rows][cols] image, the format of DSEC's
    disparity images.  filters: one PNG filter type (0 None, 1 Sub, 2 Up, 3 Average, 4 Paeth) for every scanline, or one
    per row."""
    img = np.ascontiguousarray(img)
    if img.dtype != np.uint16 or img.ndim != 2 or img.shape[0] < 1 or img.shape[1] < 1:
        raise ValueError("write_png_gray16 takes a non-empty 2-D uint16 image")
    rows, cols = img.shape
    ftypes = np.broadcast_to(np.asarray(filters, np.int64), (rows,))
    if ((ftypes < 0) | (ftypes > 4)).any():
        raise ValueError("PNG filter types are 0 .. 4")
    lines = img.astype(">u2").view(np.uint8).reshape(rows, 2 * cols).astype(np.int64)
    body = bytearray()
    prev = np.zeros(2 * cols, np.int64)
    for r in range(rows):
        cur = lines[r]
        a = np.concatenate([np.zeros(2, np.int64), cur[:-2]])        # the byte one pixel (2 bytes) to the left
        c = np.concatenate([np.zeros(2, np.int64), prev[:-2]])
        ft = int(ftypes[r])
        pred = (0, a, prev, (a + prev) // 2, _paeth(a, prev, c))[ft]
        body.append(ft)
        body += ((cur - pred) & 255).astype(np.uint8).tobytes()
        prev = cur
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + _png_chunk(b"IHDR", struct.pack(">IIBBBBB", cols, rows, 16, 0, 0, 0, 0)) +
                _png_chunk(b"IDAT", zlib.compress(bytes(body), 6)) + _png_chunk(b"IEND", b""))
    return rows, cols


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def read_png_gray16(path):
    """The uint16 [rows][cols] samples of a 16-bit grayscale PNG (colour type 0, bit depth 16, not interlaced; the five
    filter types; any number of IDAT chunks; ancillary chunks skipped), as scripts/evaluate_mcemvs_dsec.py:99 needs
    them: plt.imread gives these samples / 65535 as float32 (engine.disparity_from_png16).  Any other PNG, a bad
    checksum or a short file raises ValueError."""
    with open(path, "rb") as f:
        buf = f.read()
    if buf[:8] != b"\x89PNG\r\n\x1a\n":
        raise ValueError("%s: not a PNG file" % path)
    pos, header, data, ended = 8, None, [], False
    while pos + 12 <= len(buf) and not ended:
        (length,), kind = struct.unpack(">I", buf[pos:pos + 4]), buf[pos + 4:pos + 8]
        body = buf[pos + 8:pos + 8 + length]
        if len(body) != length or pos + 12 + length > len(buf):
            raise ValueError("%s: truncated %r chunk" % (path, kind))
        if struct.unpack(">I", buf[pos + 8 + length:pos + 12 + length])[0] != (zlib.crc32(kind + body) & 0xffffffff):
            raise ValueError("%s: bad checksum in %r chunk" % (path, kind))
        pos += 12 + length
        if kind == b"IHDR":
            if length != 13:
                raise ValueError("%s: bad IHDR" % path)
            header = struct.unpack(">IIBBBBB", body)
        elif kind == b"IDAT":
            data.append(body)
        elif kind == b"IEND":
            ended = True
        elif not (kind[0] & 0x20):
            raise ValueError("%s: unknown critical chunk %r" % (path, kind))
    if header is None or not ended:
        raise ValueError("%s: no IHDR or no IEND chunk" % path)
    cols, rows, depth, colour, compression, filt, interlace = header
    if (depth, colour) != (16, 0):
        raise ValueError("%s: bit depth %d, colour type %d: only 16-bit grayscale is read" % (path, depth, colour))
    if interlace != 0 or compression != 0 or filt != 0:
        raise ValueError("%s: interlaced or unknown compression / filter method" % path)
    if rows < 1 or cols < 1:
        raise ValueError("%s: empty image" % path)
    try:
        raw = zlib.decompress(b"".join(data))
    except zlib.error as e:
        raise ValueError("%s: %s" % (path, e))
    stride = 2 * cols
    if len(raw) != rows * (stride + 1):
        raise ValueError("%s: %d bytes of image data, expected %d" % (path, len(raw), rows * (stride + 1)))
    lines = np.frombuffer(raw, np.uint8).reshape(rows, stride + 1)
    out = np.zeros((rows, stride), np.uint8)
    prev = np.zeros(stride, np.int64)
    for r in range(rows):
        ft, x = int(lines[r, 0]), lines[r, 1:].astype(np.int64)
        if ft == 0:
            cur = x
        elif ft == 2:
            cur = (x + prev) & 255
        elif ft == 1:                                              # each of the two byte lanes is a running sum
            cur = np.empty(stride, np.int64)
            cur[0::2], cur[1::2] = np.cumsum(x[0::2]) & 255, np.cumsum(x[1::2]) & 255
        elif ft in (3, 4):                                         # the left neighbour is a reconstructed byte: serial
            cur = np.empty(stride, np.int64)
            xs, ps = x.tolist(), prev.tolist()
            line = [0] * stride
            for i in range(stride):
                a = line[i - 2] if i >= 2 else 0
                b = ps[i]
                if ft == 3:
                    pred = (a + b) >> 1
                else:
                    c = ps[i - 2] if i >= 2 else 0
                    p = a + b - c
                    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                    pred = a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)
                line[i] = (xs[i] + pred) & 255
            cur[:] = line
        else:
            raise ValueError("%s: filter type %d in row %d" % (path, ft, r))
        out[r] = cur
        prev = cur
    return out.view(">u2").astype(np.uint16)


def dsec_disparity_name(frame_id):
    """scripts/evaluate_mcemvs_dsec.py:99: the file of ground-truth frame `frame_id` in DSEC's disparity_event folder."""
    return str(int(frame_id) * 2).zfill(6) + ".png"


def save_depth_maps(out_path, suffix, depth, conf, mask, min_depth, max_depth, images=None, ctx=None, lut=None):
    """saveDepthMaps (utils.cpp:22-104): out_path + "depth_points_" + suffix + ".txt", "confidence_map_negated_" + suffix +
    ".png" and "inv_depth_colored_dilated_" + suffix + ".png" (out_path is a prefix, as in the reference).  images =
    (confidence_negated, inv_depth_colored_dilated) as engine.depth_images / MapperEMVS.depthImages return them; None
    computes them on the device of `ctx` (engine.Context) with the colour table `lut`.  Returns the three file names."""
    if images is None:
        if ctx is None:
            raise ValueError("save_depth_maps needs images, or a ctx to compute them with")
        from . import engine as _engine
        images = _engine.depth_images(ctx, depth, conf, mask, min_depth, max_depth, lut)
    neg, bgr = images
    names = [out_path + "depth_points_" + suffix + ".txt", out_path + "confidence_map_negated_" + suffix + ".png",
             out_path + "inv_depth_colored_dilated_" + suffix + ".png"]
    save_depth_points(names[0], depth, mask)
    write_png_gray8(names[1], neg)
    write_png_rgb8(names[2], bgr)
    return names


def save_depth_points(path, depth_map, mask):
    """utils.cpp:31-46: one line "c r depth" per pixel with mask > 0, row-major scan; depth is
    streamed with operator<<(float), i.e. up to 6 significant digits (%g)."""
    depth_map = np.asarray(depth_map, np.float32)
    mask = np.asarray(mask)
    rows, cols = np.nonzero(mask > 0)
    with open(path, "w") as f:
        for r, c in zip(rows, cols):
            f.write("%d %d %g\n" % (c, r, depth_map[r, c]))
    return rows.shape[0]


def load_depth_points(path, height, width, no_estimate=255.0):
    """The inverse of save_depth_points, as scripts/evaluate_mcemvs_dsec.py:69-79 reads a run's depth_points_*.txt:
    (depth float32 [height][width], mask uint8) from "col row depth" lines; a later line for a pixel replaces an earlier
    one.  A depth of exactly `no_estimate` counts as no estimate, because the script marks empty pixels with 255 and masks
    every pixel that equals it.  An empty file gives an empty mask.  Pixels outside height x width raise ValueError."""
    depth = np.zeros((int(height), int(width)), np.float32)
    mask = np.zeros((int(height), int(width)), np.uint8)
    with open(path) as f:
        vals = np.array(f.read().split(), np.float64)
    if vals.size % 3:
        raise ValueError("%s: expected lines of 'col row depth'" % path)
    pts = vals.reshape(-1, 3)
    if pts.shape[0]:
        c, r = pts[:, 0].astype(int), pts[:, 1].astype(int)
        if c.min() < 0 or r.min() < 0 or c.max() >= width or r.max() >= height:
            raise ValueError("%s: a point lies outside %d x %d" % (path, width, height))
        depth[r, c] = pts[:, 2]
        mask[r, c] = pts[:, 2] != no_estimate
        depth[mask == 0] = 0
    return depth, mask


def save_pcd_ascii(path, points):
    """What pcl::io::savePCDFileASCII(path, cloud) writes for a pcl::PointCloud<pcl::PointXYZI> of N points (main.cpp:
    397-402 saves every run's getPointcloud output so): the "# .PCD v0.7" header with FIELDS x y z intensity, SIZE 4 4 4 4,
    TYPE F F F F, COUNT 1 1 1 1, WIDTH N, HEIGHT 1, VIEWPOINT 0 0 0 1 0 0 0 (the cloud's default sensor pose), POINTS N,
    DATA ascii, then one line per point, the four values at 8 significant digits (the default precision of
    savePCDFileASCII; an ostream's default float format, i.e. %.8g; NaN as "nan").  UNPINNED: restated from PCL's
    documentation of the format, not compared with PCL's own output.  points: (N, >= 4) array, x y z intensity first.
    A world map (engine.WorldMap.extract) goes through as np.column_stack([cells["xyz"], cells["windows"]]): the number of
    windows that saw the cell as the intensity (counts below 2^24 are exact in float32)."""
    pts = np.asarray(points, np.float32)
    if pts.size == 0:
        pts = pts.reshape(0, 4)
    if pts.ndim != 2 or pts.shape[1] < 4:
        raise ValueError("points must be (N, 4): x, y, z, intensity")
    n = pts.shape[0]

    def fmt(v):
        return "nan" if np.isnan(v) else "%.8g" % float(v)

    with open(path, "w") as f:
        f.write("# .PCD v0.7 - Point Cloud Data file format\n"
                "VERSION 0.7\n"
                "FIELDS x y z intensity\n"
                "SIZE 4 4 4 4\n"
                "TYPE F F F F\n"
                "COUNT 1 1 1 1\n"
                "WIDTH %d\n"
                "HEIGHT 1\n"
                "VIEWPOINT 0 0 0 1 0 0 0\n"
                "POINTS %d\n"
                "DATA ascii\n" % (n, n))
        for p in pts[:, :4]:
            f.write(" ".join(fmt(v) for v in p) + "\n")
    return n


def pcd_curvature(evals):
    """PCL's surface variation eval0 / ((eval0 + eval1) + eval2) in float64 from rows of ascending eigenvalues (engine.
    WorldMap.fetchPca's eval); NaN where the sum is 0 or not finite (a lone or sparse cell)"""
    e = np.asarray(evals, np.float64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        total = (e[:, 0] + e[:, 1]) + e[:, 2]
        return np.where(np.isfinite(total) & (total > 0.0), e[:, 0] / total, np.nan)


_PCD_NORMAL_FIELDS = "x y z normal_x normal_y normal_z curvature"


def save_pcd_normals_ascii(path, points, normals, curvature):
    """What pcl::io::savePCDFileASCII writes for a pcl::PointCloud<pcl::PointNormal> of N points, restated from PCL's
    documentation of the format as save_pcd_ascii is: FIELDS x y z normal_x normal_y normal_z curvature, seven float32
    (NaN as "nan") at 9 significant digits -- savePCDFileASCII's precision argument, one above its default, because 8 digits
    do not bring every float32 back and a unit normal should stay one.  points and normals: (N, >= 3); curvature: N values
    -- pcd_curvature of the eigenvalues that engine.WorldMap.fetchPca returns.  Returns N."""
    pts, nrm = np.asarray(points, np.float32), np.asarray(normals, np.float32)
    cur = np.asarray(curvature, np.float64).reshape(-1).astype(np.float32)
    if pts.size == 0 and nrm.size == 0:
        pts, nrm = pts.reshape(0, 3), nrm.reshape(0, 3)
    if pts.ndim != 2 or nrm.ndim != 2 or pts.shape[1] < 3 or nrm.shape[1] < 3 or not pts.shape[0] == nrm.shape[0] == cur.shape[0]:
        raise ValueError("points and normals must be (N, 3) and curvature N values")
    n = pts.shape[0]
    rows = np.column_stack([pts[:, :3], nrm[:, :3], cur])

    def fmt(v):
        return "nan" if np.isnan(v) else "%.9g" % float(v)

    with open(path, "w") as f:
        f.write("# .PCD v0.7 - Point Cloud Data file format\n"
                "VERSION 0.7\n"
                "FIELDS %s\n"
                "SIZE 4 4 4 4 4 4 4\n"
                "TYPE F F F F F F F\n"
                "COUNT 1 1 1 1 1 1 1\n"
                "WIDTH %d\n"
                "HEIGHT 1\n"
                "VIEWPOINT 0 0 0 1 0 0 0\n"
                "POINTS %d\n"
                "DATA ascii\n" % (_PCD_NORMAL_FIELDS, n, n))
        for r in rows:
            f.write(" ".join(fmt(v) for v in r) + "\n")
    return n


def load_pcd_normals_ascii(path):
    """Reads back what save_pcd_normals_ascii wrote: dict of points (N, 3), normals (N, 3) and curvature [N], float32 (%.9g
    round-trips a float32 exactly).  Raises ValueError for any other header."""
    with open(path) as f:
        lines = f.read().split("\n")
    head = dict(l.split(" ", 1) for l in lines[1:11])
    if head.get("FIELDS") != _PCD_NORMAL_FIELDS or head.get("DATA") != "ascii" or head.get("TYPE") != "F F F F F F F":
        raise ValueError("%s: not an ascii PCD file of x y z normal_x normal_y normal_z curvature" % path)
    n = int(head["POINTS"])
    rows = np.array([[float(v) for v in l.split()] for l in lines[11:11 + n]], np.float64).reshape(n, 7).astype(np.float32)
    return {"points": rows[:, :3], "normals": rows[:, 3:6], "curvature": rows[:, 6]}


_MAP_SCALARS = (("leaf", np.float64), ("calls", np.uint64), ("accepted", np.uint64), ("rejected", np.uint64))
_MAP_ARRAYS = (("keys", np.uint64, 1), ("n", np.uint32, 1), ("S", np.uint64, 2), ("windows", np.uint32, 1), ("stamp", np.uint32, 1))


def save_world_map(path, state):
    """A world map's exact state (engine.WorldMap.exportState) as one .npz file, with numpy alone: leaf (float64), calls,
    accepted, rejected (uint64) and per cell keys (uint64), n (uint32), S (uint64, (M, 3)), windows and stamp (uint32).
    Written to exactly `path` (no ".npz" is appended).  load_world_map reads it back; WorldMap.importState of that into
    an empty map restores the map bit for bit."""
    out = {k: np.asarray(state[k], t).reshape(()) for k, t in _MAP_SCALARS}
    for k, t, ndim in _MAP_ARRAYS:
        a = np.asarray(state[k])
        if a.dtype != t or a.ndim != ndim:
            raise ValueError("%s must be %s with %d dimension(s) (got %s, %s)" % (k, np.dtype(t).name, ndim, a.dtype.name, a.shape))
        out[k] = a
    _check_world_map_shapes(out)
    with open(path, "wb") as f:
        np.savez(f, **out)


def _check_world_map_shapes(a):
    m = a["keys"].shape[0]
    if a["S"].shape != (m, 3) or any(a[k].shape != (m,) for k in ("n", "windows", "stamp")):
        raise ValueError("keys, n, windows and stamp need one entry per cell and S three: got %s"
                         % {k: a[k].shape for k, _, _ in _MAP_ARRAYS})


def load_world_map(path):
    """The state save_world_map wrote, as exportState returns it (Python numbers for leaf, calls, accepted, rejected).
    ValueError for a missing entry, a wrong dtype or a wrong shape: nothing is converted."""
    with np.load(path, allow_pickle=False) as z:
        missing = [k for k, _ in _MAP_SCALARS] + [k for k, _, _ in _MAP_ARRAYS]
        missing = [k for k in missing if k not in z.files]
        if missing:
            raise ValueError("not a world map file: %s missing" % ", ".join(missing))
        a = {k: z[k] for k in z.files}
    for k, t in _MAP_SCALARS:
        if a[k].dtype != t or a[k].shape != ():
            raise ValueError("%s must be a %s scalar (got %s, %s)" % (k, np.dtype(t).name, a[k].dtype.name, a[k].shape))
    for k, t, ndim in _MAP_ARRAYS:
        if a[k].dtype != t or a[k].ndim != ndim:
            raise ValueError("%s must be %s with %d dimension(s) (got %s, %s)" % (k, np.dtype(t).name, ndim, a[k].dtype.name, a[k].shape))
    _check_world_map_shapes(a)
    out = {"leaf": float(a["leaf"]), "calls": int(a["calls"]), "accepted": int(a["accepted"]), "rejected": int(a["rejected"])}
    out.update({k: a[k] for k, _, _ in _MAP_ARRAYS})
    return out


# ------------------------------------------------------------------ ROSBAG v2.0 (subset)
_MAGIC = b"#ROSBAG V2.0\n"
_OP_MSG, _OP_BAG_HEADER, _OP_INDEX, _OP_CHUNK, _OP_CHUNK_INFO, _OP_CONN = 2, 3, 4, 5, 6, 7


def _read_fields(buf):
    fields, i = {}, 0
    while i < len(buf):
        (n,) = struct.unpack_from("<I", buf, i)
        i += 4
        name, _, val = buf[i:i + n].partition(b"=")
        fields[name.decode()] = val
        i += n
    return fields


def _records(buf, start=0, end=None):
    i = start
    end = len(buf) if end is None else end
    while i + 8 <= end:
        (hl,) = struct.unpack_from("<I", buf, i)
        header = _read_fields(buf[i + 4:i + 4 + hl])
        i += 4 + hl
        (dl,) = struct.unpack_from("<I", buf, i)
        yield header, buf[i + 4:i + 4 + dl]
        i += 4 + dl


def _scan_bag(path, on_message):
    """Walks every message record of a ROSBAG v2.0 file (chunks with compression none or bz2) in
    file order and calls on_message(topic, type, data)."""
    buf = open(path, "rb").read()
    if not buf.startswith(_MAGIC):
        raise ValueError("%s is not a ROSBAG V2.0 file" % path)
    conns = {}

    def handle(header, data):
        op = header["op"][0]
        if op == _OP_CONN:
            conn = struct.unpack("<I", header["conn"])[0]
            info = _read_fields(data)
            conns[conn] = (header["topic"].decode(), info.get("type", b"").decode())
        elif op == _OP_MSG:
            conn = struct.unpack("<I", header["conn"])[0]
            tpc, typ = conns.get(conn, ("", ""))
            return on_message(tpc, typ, data)
        return True

    for header, data in _records(buf, len(_MAGIC)):
        op = header["op"][0]
        if op == _OP_CHUNK:
            comp = header.get("compression", b"none")
            if comp == b"bz2":
                data = bz2.decompress(data)
            elif comp != b"none":
                raise ValueError("chunk compression %r is not supported (none, bz2)" % comp)
            for h2, d2 in _records(data):
                if handle(h2, d2) is False:
                    return
        elif handle(header, data) is False:
            return


def _parse_pose_stamped(data):
    """std_msgs/Header (seq, stamp.sec, stamp.nsec, frame_id) + geometry_msgs/Pose."""
    seq, sec, nsec, n = struct.unpack_from("<IIII", data, 0)
    off = 16 + n
    px, py, pz, qx, qy, qz, qw = struct.unpack_from("<7d", data, off)
    return sec + 1e-9 * nsec, (px, py, pz, qw, qx, qy, qz)


def read_pose_bag(path, topic=None):
    """Reads geometry_msgs/PoseStamped messages of a ROSBAG v2.0 file.
    Returns (times float64[n] by header stamp, poses float64[n][7] = tx,ty,tz,qw,qx,qy,qz),
    sorted by time like the reference's std::map<ros::Time, Transformation>."""
    out = []

    def on_message(tpc, typ, data):
        if (topic is None or tpc == topic) and typ == "geometry_msgs/PoseStamped":
            out.append(_parse_pose_stamped(data))
        return True

    _scan_bag(path, on_message)
    out.sort(key=lambda tp: tp[0])
    times = np.array([t for t, _ in out], np.float64)
    poses = np.array([p for _, p in out], np.float64).reshape(-1, 7)
    return times, poses


def parse_rosbag_gt(path, topic=None, tmin=0.0, tmax=float("inf")):
    """data_loading::parse_rosbag_gt (data_loading.cpp:303-420) for PoseStamped bags: the stamps of the
    returned control poses are RELATIVE to the first pose message of the topic (`initial_timestamp`,
    :339-343 -- the same convention parse_rosbag applies to the events, :262-268, so that events and
    poses share a time axis starting at ~0); poses with relative stamp < tmin are skipped, the first
    one beyond tmax is still taken and ends the scan (:346-353, the flag is tested at the next
    message).  read_pose_bag() above keeps the absolute stamps instead.
    Returns (times float64[n], poses float64[n][7] = tx,ty,tz,qw,qx,qy,qz), in bag order."""
    out = []
    state = {"t0": None, "go": True}

    def on_message(tpc, typ, data):
        if not state["go"]:
            return False
        if (topic is None or tpc == topic) and typ == "geometry_msgs/PoseStamped":
            t, p = _parse_pose_stamped(data)
            if state["t0"] is None:
                state["t0"] = t
            rel = t - state["t0"]
            if rel < tmin:
                return True
            if rel > tmax:
                state["go"] = False
            out.append((rel, p))
        return True

    _scan_bag(path, on_message)
    # the reference keeps them in a std::map<ros::Time, Transformation> filled with insert(): ascending by stamp,
    # and of several poses with the SAME stamp only the first one is kept (insert does not overwrite)
    out.sort(key=lambda tp: tp[0])          # stable: equal stamps stay in bag order
    out = [tp for i, tp in enumerate(out) if i == 0 or tp[0] != out[i - 1][0]]
    times = np.array([t for t, _ in out], np.float64)
    poses = np.array([p for _, p in out], np.float64).reshape(-1, 7)
    return times, poses


def _field(name, val):
    body = name.encode() + b"=" + val
    return struct.pack("<I", len(body)) + body


def _record(fields, data):
    header = b"".join(_field(k, v) for k, v in fields)
    return struct.pack("<I", len(header)) + header + struct.pack("<I", len(data)) + data


def write_pose_bag(path, times, poses, topic="/pose", frame_id="world"):
    """Minimal single-chunk, uncompressed ROSBAG v2.0 with PoseStamped messages (no index
    records: readers that scan chunks, like read_pose_bag, accept it).  Test helper."""
    conn = struct.pack("<I", 0)
    conn_data = b"".join(_field(k, v) for k, v in (
        ("topic", topic.encode()), ("type", b"geometry_msgs/PoseStamped"),
        ("md5sum", b"d3812c3cbc69362b77dc0b19b345f8f5"), ("message_definition", b"")))
    recs = [_record((("op", bytes([_OP_CONN])), ("conn", conn), ("topic", topic.encode())), conn_data)]
    for seq, (t, p) in enumerate(zip(times, poses)):
        sec = int(np.floor(t))
        nsec = int(round((t - sec) * 1e9))
        if nsec >= 1000000000:
            sec, nsec = sec + 1, nsec - 1000000000
        fid = frame_id.encode()
        msg = struct.pack("<IIII", seq, sec, nsec, len(fid)) + fid + struct.pack(
            "<7d", p[0], p[1], p[2], p[4], p[5], p[6], p[3])
        recs.append(_record((("op", bytes([_OP_MSG])), ("conn", conn),
                             ("time", struct.pack("<II", sec, nsec))), msg))
    chunk = b"".join(recs)
    bag_header = _record((("op", bytes([_OP_BAG_HEADER])), ("index_pos", struct.pack("<Q", 0)),
                          ("conn_count", struct.pack("<I", 1)), ("chunk_count", struct.pack("<I", 1))), b"")
    pad = 4096 - len(_MAGIC) - len(bag_header)
    if pad > 0:  # rosbag pads the bag header record to 4096 bytes
        bag_header = bag_header[:-4] + struct.pack("<I", pad) + b" " * pad
    with open(path, "wb") as f:
        f.write(_MAGIC + bag_header)
        f.write(_record((("op", bytes([_OP_CHUNK])), ("compression", b"none"),
                         ("size", struct.pack("<I", len(chunk)))), chunk))


# dvs_msgs/Event as serialised by ROS: uint16 x, uint16 y, time ts (u32 sec, u32 nsec), bool polarity
_EVENT_DTYPE = np.dtype([("x", "<u2"), ("y", "<u2"), ("sec", "<u4"), ("nsec", "<u4"), ("p", "u1")])


def _parse_event_array(data):
    """std_msgs/Header, uint32 height, uint32 width, dvs_msgs/Event[] events."""
    (n,) = struct.unpack_from("<I", data, 12)
    off = 16 + n
    height, width, count = struct.unpack_from("<III", data, off)
    ev = np.frombuffer(data, _EVENT_DTYPE, count, off + 12)
    return height, width, ev


def read_event_bag(path, topic, tmin=0.0, tmax=float("inf"), events_offset=0.0):
    """parse_rosbag's event branch (data_loading.cpp:66-104) + the final sort (:211-216).
    The first event of the first non-empty message defines the initial stamp; an event is kept
    iff its stamp relative to that is >= tmin; the message in which a relative stamp exceeds tmax
    is still taken whole (the reference only stops reading AFTER it); timestamps become
    ts - initial - events_offset (seconds, double); events are sorted by timestamp.
    Returns dict(x u16[n], y u16[n], ts f64[n], polarity u8[n], height, width, initial_stamp)."""
    xs, ys, tss, ps = [], [], [], []
    state = {"t0": None, "h": 0, "w": 0}

    def on_message(tpc, typ, data):
        if tpc != topic or typ != "dvs_msgs/EventArray":
            return True
        h, w, ev = _parse_event_array(data)
        if ev.shape[0] == 0:
            return True
        state["h"], state["w"] = h, w
        if state["t0"] is None:
            state["t0"] = (int(ev["sec"][0]), int(ev["nsec"][0]))
        s0, n0 = state["t0"]
        # (ts - initial).toSec() on ros::Duration: exact integer nanoseconds -> double
        rel_ns = (ev["sec"].astype(np.int64) - s0) * 1000000000 + (ev["nsec"].astype(np.int64) - n0)
        rel = rel_ns.astype(np.float64) * 1e-9
        keep = rel >= tmin
        # ev.ts.toSec() - initial.toSec() - offset, each toSec() = sec + 1e-9 * nsec in double
        t_abs = ev["sec"].astype(np.float64) + 1e-9 * ev["nsec"].astype(np.float64)
        t_new = t_abs - (float(s0) + 1e-9 * float(n0)) - events_offset
        xs.append(ev["x"][keep])
        ys.append(ev["y"][keep])
        tss.append(t_new[keep])
        ps.append(ev["p"][keep])
        return not bool(np.any(rel > tmax))   # stop after this message

    _scan_bag(path, on_message)
    if not xs:
        z = np.empty(0)
        return {"x": z.astype(np.uint16), "y": z.astype(np.uint16), "ts": z.astype(np.float64),
                "polarity": z.astype(np.uint8), "height": 0, "width": 0, "initial_stamp": None}
    x = np.concatenate(xs)
    y = np.concatenate(ys)
    ts = np.concatenate(tss)
    p = np.concatenate(ps)
    order = np.argsort(ts, kind="stable")
    t0 = state["t0"]
    return {"x": x[order], "y": y[order], "ts": ts[order], "polarity": p[order],
            "height": state["h"], "width": state["w"], "initial_stamp": t0[0] + 1e-9 * t0[1]}


def write_event_bag(path, x, y, ts, polarity=None, topic="/dvs/events", height=260, width=346,
                    events_per_message=5000, compression="none"):
    """Minimal ROSBAG v2.0 with dvs_msgs/EventArray messages (one chunk per message, optional
    bz2).  ts: absolute seconds (float64), written as (sec, nsec).  Test helper."""
    x = np.asarray(x, np.uint16)
    y = np.asarray(y, np.uint16)
    ts = np.asarray(ts, np.float64)
    pol = np.ones(x.shape[0], np.uint8) if polarity is None else np.asarray(polarity, np.uint8)
    sec = np.floor(ts).astype(np.int64)
    nsec = np.rint((ts - sec) * 1e9).astype(np.int64)
    carry = nsec >= 1000000000
    sec, nsec = sec + carry, nsec - carry * 1000000000
    conn = struct.pack("<I", 0)
    conn_data = b"".join(_field(k, v) for k, v in (
        ("topic", topic.encode()), ("type", b"dvs_msgs/EventArray"),
        ("md5sum", b"5e8beee5a6c107e504c2e78903c224b8"), ("message_definition", b"")))
    conn_rec = _record((("op", bytes([_OP_CONN])), ("conn", conn), ("topic", topic.encode())), conn_data)
    chunks = []
    n = x.shape[0]
    for seq, a in enumerate(range(0, max(n, 1), events_per_message)):
        b = min(n, a + events_per_message)
        ev = np.empty(b - a, _EVENT_DTYPE)
        ev["x"], ev["y"], ev["sec"], ev["nsec"], ev["p"] = x[a:b], y[a:b], sec[a:b], nsec[a:b], pol[a:b]
        hs, hn = (int(sec[a]), int(nsec[a])) if b > a else (0, 0)
        msg = struct.pack("<IIII", seq, hs, hn, 0) + struct.pack("<III", height, width, b - a) + ev.tobytes()
        rec = _record((("op", bytes([_OP_MSG])), ("conn", conn), ("time", struct.pack("<II", hs, hn))), msg)
        body = (conn_rec if seq == 0 else b"") + rec
        raw_len = len(body)
        if compression == "bz2":
            body = bz2.compress(body)
        chunks.append(_record((("op", bytes([_OP_CHUNK])), ("compression", compression.encode()),
                               ("size", struct.pack("<I", raw_len))), body))
    bag_header = _record((("op", bytes([_OP_BAG_HEADER])), ("index_pos", struct.pack("<Q", 0)),
                          ("conn_count", struct.pack("<I", 1)),
                          ("chunk_count", struct.pack("<I", len(chunks)))), b"")
    pad = 4096 - len(_MAGIC) - len(bag_header)
    if pad > 0:
        bag_header = bag_header[:-4] + struct.pack("<I", pad) + b" " * pad
    with open(path, "wb") as f:
        f.write(_MAGIC + bag_header)
        for c in chunks:
            f.write(c)
