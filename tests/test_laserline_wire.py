"""CPU tests (no GPU): SensorData.depth_image on the wire - uzl_wire_sensor_depth reads a DepthImage SensorData and the pinhole intrinsics
of its CameraInfo, uzl_wire_depth_sensor_encode writes one as SensorData::toMsg + DepthImageData::toMsg do
(graph_slam_common/src/sensor_data.cpp:40-49, 194-212), uzl_wire_depth_image turns it into what uzl_laserline_extract takes; the
expected bytes are built here with struct from SensorData.msg, sensor_msgs/Image and sensor_msgs/CameraInfo."""
import ctypes as C
import struct

import numpy as np
import pytest

from uzliti_slam_amd import capi, wire as W


def _str(s):
    s = s if isinstance(s, bytes) else s.encode()
    return struct.pack("<I", len(s)) + s


def image_bytes(im):
    """sensor_msgs/Image: header, height, width, encoding, is_bigendian, step, data"""
    return (struct.pack("<III", im["seq"], im["stamp_sec"], im["stamp_nsec"]) + _str(im["frame_id"]) +
            struct.pack("<II", im["height"], im["width"]) + _str(im["encoding"]) + struct.pack("<BI", im["is_bigendian"], im["step"]) +
            struct.pack("<I", len(im["data"])) + im["data"])


def camera_info_bytes(width, height, P, binning=(0, 0), roi=(0, 0, 0, 0, 0), D=(0.1, -0.2, 0.0, 0.0, 0.05)):
    """sensor_msgs/CameraInfo: header, height, width, distortion_model, D[], K, R, P, binning_x, binning_y, roi"""
    K = [P[0], 0, P[2], 0, P[5], P[6], 0, 0, 1]
    return (struct.pack("<III", 3, 1400000002, 5) + _str("camera_rgb_optical_frame") + struct.pack("<II", height, width) + _str("plumb_bob") +
            struct.pack("<I", len(D)) + struct.pack("<%dd" % len(D), *D) + struct.pack("<9d", *K) +
            struct.pack("<9d", 1, 0, 0, 0, 1, 0, 0, 0, 1) + struct.pack("<12d", *P) + struct.pack("<II", *binning) +
            struct.pack("<IIIIB", *roi))


DEFAULT_IMAGE = bytes(16 + 8 + 4 + 1 + 4 + 4)
DEFAULT_CAMERA_INFO = bytes(16 + 8 + 4 + 4 + 240 + 8 + 17)
DEFAULT_SCAN = bytes(16 + 28 + 4 + 4)


def depth_sensor_bytes(sec, nsec, frame, pos, depth, color=None, camera_info=None, scan=DEFAULT_SCAN + bytes(24)):
    """graph_slam_msgs/SensorData of a DepthImageData with displacement = translation pos (identity rotation)"""
    b = struct.pack("<III", 0, sec, nsec) + _str(frame)                               # header
    b += struct.pack("<i", 2)                                                          # sensor_type = SENSOR_TYPE_DEPTH_IMAGE
    b += struct.pack("<7d", pos[0], pos[1], pos[2], 0.0, 0.0, 0.0, 1.0)                 # displacement
    b += _str(frame)                                                                   # sensor_frame
    b += bytes(16) + struct.pack("<iI", 0, 0)                                          # features: header, descriptor_type, []
    b += camera_info if camera_info is not None else DEFAULT_CAMERA_INFO               # features.camera_model
    b += image_bytes(depth) + (color if color is not None else DEFAULT_IMAGE)          # depth_image: depth, color
    b += struct.pack("<I", 0)                                                          # gist_descriptor
    return b + scan                                                                    # scan, scan_center


P = [525.0, 0.0, 319.5, 0.0, 0.0, 520.0, 239.5, 0.0, 0.0, 0.0, 1.0, 0.0]


def _depth(encoding, rng, pad=0):
    """a 4 x 3 depth image, rows padded by `pad` bytes"""
    dt = np.dtype("<u2") if encoding == "16UC1" else np.dtype("<f4")
    px = rng.integers(0, 5000, (3, 4)).astype(dt) if encoding == "16UC1" else rng.uniform(0, 5, (3, 4)).astype(dt)
    rows = [px[r].tobytes() + bytes(range(1, pad + 1)) for r in range(3)]
    return dict(seq=9, stamp_sec=1400000003, stamp_nsec=77, frame_id="camera_depth_optical_frame", height=3, width=4, encoding=encoding,
                is_bigendian=0, step=4 * dt.itemsize + pad, data=b"".join(rows)), px


def _disp(pos):
    T = np.eye(3, 4)
    T[:, 3] = pos
    return T.reshape(12)


def _node(sensors):
    return dict(id="1400000003.5", stamps_ns=[1400000003 * 10**9 + 77], pose=np.eye(3, 4).reshape(12), odom_pose=np.eye(3, 4).reshape(12),
                sensors=sensors, edge_ids=["e0"], fixed=0, uncertainty=0.0)


def _decoded(raw):
    return W.decode_node(W.encode_node(_node([dict(raw=raw)])))


@pytest.mark.parametrize("encoding,pad", [("16UC1", 0), ("32FC1", 0), ("16UC1", 6), ("32FC1", 4)])
def test_decode_field_for_field(encoding, pad):
    rng = np.random.default_rng(0)
    im, px = _depth(encoding, rng, pad)
    color = image_bytes(dict(im, encoding="rgb8", step=12, data=bytes(range(36)), frame_id="camera_rgb_optical_frame"))
    ci = camera_info_bytes(640, 480, P)
    raw = depth_sensor_bytes(1400000003, 77, "camera_depth_optical_frame", [0.1, 0.0, 0.3], im, color, ci)
    d = _decoded(raw)
    s = d.fields["sensors"][0]
    assert s["sensor_type"] == W.SENSOR_TYPE_DEPTH_IMAGE and s["raw"] == raw and s["sensor_frame"] == b"camera_depth_optical_frame"
    assert np.array_equal(s["displacement"], _disp([0.1, 0.0, 0.3])) and s["camera_info"] == ci
    T = np.arange(12.0)
    got = W.sensor_depth(d.sensors_c[0], camera_transform=T, group=4)
    for k in ("seq", "stamp_sec", "stamp_nsec", "height", "width", "step", "is_bigendian", "data"):
        assert got[k] == im[k], k
    assert got["frame_id"] == im["frame_id"].encode() and got["encoding"] == encoding.encode() and got["color"] == color
    assert (got["fx"], got["fy"], got["cx"], got["cy"]) == (525.0, 520.0, 319.5, 239.5)
    g = got["image"]
    assert g["depth"].dtype == px.dtype and np.array_equal(g["depth"], px) and g["group"] == 4
    assert (g["fx"], g["fy"], g["cx"], g["cy"]) == (525.0, 520.0, 319.5, 239.5) and np.array_equal(g["camera_transform"], T)
    arr, keep = capi.Laserline.pack_images([g])                                      # what extract would be handed: strided rows, no copy
    assert (arr[0].width, arr[0].height, arr[0].step, arr[0].encoding) == (4, 3, im["step"], 1 if encoding == "16UC1" else 0)


@pytest.mark.parametrize("encoding", ["16UC1", "32FC1"])
def test_encoder_writes_the_message_byte_for_byte(encoding):
    rng = np.random.default_rng(1)
    im, _ = _depth(encoding, rng, pad=2)
    color = image_bytes(dict(im, encoding="rgb8", step=12, data=bytes(range(36))))
    ci = camera_info_bytes(640, 480, P)
    for col, cam in ((None, None), (color, None), (None, ci), (color, ci)):
        want = depth_sensor_bytes(7, 8, "cam", [1.5, -2.0, 0.25], im, col, cam)
        assert W.encode_depth_sensor(7, 8, "cam", _disp([1.5, -2.0, 0.25]), dict(im, color=col), cam) == want


def test_round_trip_and_node_re_encode():
    rng = np.random.default_rng(2)
    im, px = _depth("32FC1", rng)
    ci = camera_info_bytes(4, 3, P)
    raw = W.encode_depth_sensor(1400000003, 77, "cam", _disp([0.2, 0.0, 0.0]), im, ci)
    gist = W.encode_gist_sensor(1400000003, 77, "cam", _disp([0, 0, 0]), np.arange(32, dtype=np.uint8))
    b1 = W.encode_node(_node([dict(raw=gist), dict(raw=raw)]))
    d1 = W.decode_node(b1)
    got = W.sensor_depth(d1.sensors_c[1])
    for k in ("seq", "stamp_sec", "stamp_nsec", "height", "width", "step", "is_bigendian", "data"):
        assert got[k] == im[k], k
    assert got["color"] == DEFAULT_IMAGE and got["fx"] == 525.0
    again = W.encode_depth_sensor(1400000003, 77, "cam", _disp([0.2, 0.0, 0.0]), got, d1.fields["sensors"][1]["camera_info"])
    assert again == raw
    empty = W.sensor_depth(d1.sensors_c[0])                                           # a GIST sensor's depth image is empty
    assert empty["height"] == empty["width"] == 0 and empty["data"] == b"" and empty["fx"] == 0.0
    b2 = W.encode_node(dict(d1.fields, id=d1.fields["id"].decode(), edge_ids=[e.decode() for e in d1.fields["edge_ids"]],
                            sensors=[dict(raw=x["raw"]) for x in d1.fields["sensors"]]))
    assert b2 == b1


def test_the_scan_behind_a_depth_image_is_still_found():
    rng = np.random.default_rng(3)
    im, _ = _depth("16UC1", rng, pad=2)
    r = rng.uniform(0.5, 6, 720).astype("<f4")
    scan = (struct.pack("<III", 1, 2, 3) + _str("/base_footprint") + struct.pack("<7f", -3.1, 3.1, 0.01, 0, 1 / 30, 0.45, 5.0) +
            struct.pack("<I", 720) + r.tobytes() + struct.pack("<I", 0) + struct.pack("<3d", 0.5, -1.0, 0.0))
    raw = depth_sensor_bytes(5, 6, "cam", [0, 0, 0], im, None, camera_info_bytes(4, 3, P), scan)
    d = _decoded(raw)
    sc = W.sensor_scan(d.sensors_c[0])
    assert sc["ranges"].tobytes() == r.tobytes() and sc["frame_id"] == b"/base_footprint" and sc["scan_center"].tolist() == [0.5, -1.0, 0.0]
    assert W.sensor_depth(d.sensors_c[0])["data"] == im["data"]


def test_every_truncation_point():
    rng = np.random.default_rng(4)
    im, _ = _depth("16UC1", rng)
    raw = depth_sensor_bytes(5, 6, "cam", [0, 0, 0], im, None, camera_info_bytes(4, 3, P))
    d = _decoded(raw)
    L = W._lib()
    out = W.WireDepth()
    assert L.uzl_wire_sensor_depth(C.byref(d.sensors_c[0]), C.byref(out)) == 0
    for n in range(len(raw)):
        w = W.WireSensor(); w.raw = W.Span(d.sensors_c[0].raw.p, n)
        assert L.uzl_wire_sensor_depth(C.byref(w), C.byref(out)) == W.UZL_ERR_TRUNCATED, n
    assert L.uzl_wire_sensor_depth(C.byref(d.sensors_c[0]), None) == -1 and L.uzl_wire_sensor_depth(None, C.byref(out)) == -1
    # data shorter than height * step: the message parses, the image form does not
    short = dict(im, data=im["data"][:-1])
    d = _decoded(depth_sensor_bytes(5, 6, "cam", [0, 0, 0], short, None, camera_info_bytes(4, 3, P)))
    with pytest.raises(capi.UzlError) as e:
        W.sensor_depth(d.sensors_c[0], camera_transform=np.eye(3, 4))
    assert e.value.status == W.UZL_ERR_TRUNCATED
    # encode into a buffer that is too small
    buf = (C.c_uint8 * 64)(); wr = C.c_uint64(0)
    k = W._Keep()
    w = W.WireDepth(); w.data = k.span(bytes(100)); w.height, w.width, w.step = 5, 10, 20
    disp = (C.c_double * 12)(*_disp([0, 0, 0]))
    assert L.uzl_wire_depth_sensor_encode(1, 2, W.Span(None, 0), disp, C.byref(w), W.Span(None, 0), buf, 64, C.byref(wr)) == W.UZL_ERR_TRUNCATED
    assert wr.value == L.uzl_wire_depth_sensor_size(W.Span(None, 0), C.byref(w), W.Span(None, 0)) > 64
    w.data = W.Span(None, 5)                                                          # a length without bytes
    assert L.uzl_wire_depth_sensor_size(W.Span(None, 0), C.byref(w), W.Span(None, 0)) == 0
    assert L.uzl_wire_depth_sensor_encode(1, 2, W.Span(None, 0), disp, C.byref(w), W.Span(None, 0), buf, 64, C.byref(wr)) == -1


@pytest.mark.parametrize("what", ["roi", "binning", "mono8", "bigendian"])
def test_unsupported(what):
    rng = np.random.default_rng(5)
    im, _ = _depth("16UC1", rng)
    ci = camera_info_bytes(4, 3, P, binning=(2, 2) if what == "binning" else (1, 1), roi=(1, 1, 2, 2, 0) if what == "roi" else (0, 0, 0, 0, 1))
    if what == "mono8":
        im = dict(im, encoding="mono8", step=4, data=bytes(12))
    if what == "bigendian":
        im = dict(im, is_bigendian=1)
    d = _decoded(depth_sensor_bytes(5, 6, "cam", [0, 0, 0], im, None, ci))
    if what in ("mono8", "bigendian"):
        assert W.sensor_depth(d.sensors_c[0])["encoding"] == im["encoding"].encode()  # the message itself decodes
    with pytest.raises(capi.UzlError) as e:
        W.sensor_depth(d.sensors_c[0], camera_transform=np.eye(3, 4))
    assert e.value.status == W.UZL_ERR_UNSUPPORTED


def test_depth_parser_under_address_and_ub_sanitizers(tmp_path):
    """100k mutated / truncated Node messages with depth-image sensors through an ASan + UBSan build of the host-side codec
    (sanitizers run on the CPU build only)."""
    import os
    import shutil
    import subprocess
    if not shutil.which("g++"):
        pytest.skip("no g++")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rng = np.random.default_rng(6)
    seeds = []
    for k, (encoding, pad) in enumerate([("16UC1", 0), ("32FC1", 4)]):
        im, _ = _depth(encoding, rng, pad)
        color = image_bytes(dict(im, encoding="rgb8", step=12, data=bytes(range(36))))
        raw = depth_sensor_bytes(5, 6, "cam", [0.1, 0.2, 0.3], im, color if k else None, camera_info_bytes(4, 3, P))
        gist = W.encode_gist_sensor(5, 6, "cam", _disp([0, 0, 0]), np.arange(32, dtype=np.uint8))
        p = tmp_path / ("node%d.bin" % k); p.write_bytes(W.encode_node(_node([dict(raw=raw), dict(raw=gist)]))); seeds.append(str(p))
    exe = str(tmp_path / "fuzz_wire_depth")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-x", "c++",
                           os.path.join(root, "uzliti_slam_amd", "csrc", "uzl_wire.hip"), os.path.join(root, "tests", "fuzz_wire_depth.cpp"),
                           "-o", exe])
    out = subprocess.run([exe] + seeds, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "fuzz: 100000 inputs" in out.stdout
    counts = [int(x) for x in out.stdout.split("node")[1].replace("depth", "").replace("image", "").split()]
    assert min(counts) > 1000, out.stdout
