"""CPU tests (no GPU): SensorData.gist_descriptor on the wire - uzl_wire_sensor_gist reads it from a decoded sensor,
uzl_wire_gist_sensor_encode writes a SENSOR_TYPE_BINARY_GIST SensorData as SensorData::toMsg + BinaryGistData::toMsg do
(graph_slam_common/src/sensor_data.cpp:40-49, 227-246).  The expected bytes are built here with struct from SensorData.msg."""
import struct

import numpy as np
import pytest

from oracle import wire as OW
from uzliti_slam_amd import wire as W


def gist_sensor_bytes(sec, nsec, frame, pos, floats):
    """graph_slam_msgs/SensorData of a BinaryGistData with displacement = translation pos (identity rotation)"""
    f = frame.encode()
    b = struct.pack("<III", 0, sec, nsec) + struct.pack("<I", len(f)) + f           # header
    b += struct.pack("<i", 3)                                                          # sensor_type = SENSOR_TYPE_BINARY_GIST
    b += struct.pack("<7d", pos[0], pos[1], pos[2], 0.0, 0.0, 0.0, 1.0)                 # displacement: position, orientation xyzw
    b += struct.pack("<I", len(f)) + f                                                 # sensor_frame
    b += bytes(16) + struct.pack("<iI", 0, 0)                                          # features: header, descriptor_type, []
    b += bytes(16 + 8 + 4 + 4 + 240 + 8 + 17)                                          # features.camera_model (CameraInfo)
    b += bytes(2 * (16 + 8 + 4 + 1 + 4 + 4))                                           # depth_image: depth, color (Image)
    b += struct.pack("<I", len(floats)) + np.asarray(floats, "<f4").tobytes()          # gist_descriptor
    b += bytes(16 + 28 + 4 + 4)                                                        # scan (LaserScan)
    b += bytes(24)                                                                     # scan_center
    return b


def _disp(pos):
    T = np.eye(3, 4)
    T[:, 3] = pos
    return T.reshape(12)


def _feature_sensor(rng):
    desc = rng.integers(0, 256, size=(20, 32), dtype=np.uint8)
    pos = rng.normal(size=(3, 20)); valid = np.ones(20, np.uint8); uv = rng.integers(0, 640, size=(20, 2)).astype(np.int32)
    return dict(raw=None, sensor_type=1, stamp_sec=1400000000, stamp_nsec=7, sensor_frame="camera_rgb_optical_frame",
                displacement=_disp([0.1, 0.2, 0.3]), descriptor_type=2, n_features=20, desc_len=32,
                records=OW.features_pack(desc, pos, valid, uv), camera_info=None)


def _node(sensors):
    return dict(id="1400000000.5", stamps_ns=[1400000000 * 10**9 + 5], pose=np.eye(3, 4).reshape(12), odom_pose=np.eye(3, 4).reshape(12),
                sensors=sensors, edge_ids=["e0"], fixed=0, uncertainty=0.0)


def test_decode_node_with_feature_and_gist_sensors():
    rng = np.random.default_rng(0)
    gist = rng.integers(0, 256, 32, dtype=np.uint8)
    raw = gist_sensor_bytes(1400000000, 9, "camera_rgb_optical_frame", [1.0, 2.0, 3.0], gist.astype(np.float32))
    d = W.decode_node(W.encode_node(_node([_feature_sensor(rng), dict(raw=raw)])))
    s = d.fields["sensors"]
    assert [x["sensor_type"] for x in s] == [W.SENSOR_TYPE_FEATURE, W.SENSOR_TYPE_BINARY_GIST]
    assert s[1]["raw"] == raw and s[1]["stamp_nsec"] == 9 and s[1]["sensor_frame"] == b"camera_rgb_optical_frame"
    assert np.array_equal(W.sensor_gist(d.sensors_c[1]), gist)
    assert len(W.sensor_gist(d.sensors_c[0])) == 0                                   # a FEATURE sensor's gist_descriptor is empty


def test_encoder_writes_the_message_byte_for_byte():
    gist = np.arange(32, dtype=np.uint8) * 7
    want = gist_sensor_bytes(1400000123, 456, "cam", [1.5, -2.0, 0.25], gist.astype(np.float32))
    assert W.encode_gist_sensor(1400000123, 456, "cam", _disp([1.5, -2.0, 0.25]), gist) == want
    assert W.encode_gist_sensor(0, 0, "", np.eye(3, 4), np.zeros(0, np.uint8)) == gist_sensor_bytes(0, 0, "", [0, 0, 0], [])


def test_round_trip_and_node_re_encode_keeps_the_gist_sensor():
    rng = np.random.default_rng(1)
    for nbytes in (32, 64, 1):
        gist = rng.integers(0, 256, nbytes, dtype=np.uint8)
        raw = W.encode_gist_sensor(1400000000, 1, "kinect", _disp([3.0, 0.0, -1.0]), gist)
        b1 = W.encode_node(_node([_feature_sensor(rng), dict(raw=raw)]))
        d1 = W.decode_node(b1)
        assert np.array_equal(W.sensor_gist(d1.sensors_c[1]), gist)
        assert np.array_equal(d1.fields["sensors"][1]["displacement"], _disp([3.0, 0.0, -1.0]))
        # decode -> encode (raw copied through) -> decode: the GIST sensor keeps every byte
        b2 = W.encode_node(dict(d1.fields, id=d1.fields["id"].decode(), edge_ids=[e.decode() for e in d1.fields["edge_ids"]],
                                sensors=[dict(raw=x["raw"]) for x in d1.fields["sensors"]]))
        assert b2 == b1
        d2 = W.decode_node(b2)
        assert d2.fields["sensors"][1]["raw"] == raw and np.array_equal(W.sensor_gist(d2.sensors_c[1]), gist)


def test_floats_outside_0_255_follow_the_feature_rule():
    vals = np.array([0.0, 255.0, 255.9, 256.0, 257.5, -1.0, -0.5, 3e9, np.nan, -3e9, 1e-30, 65535.0, -256.0, 2147483520.0],
                    np.float32)
    raw = gist_sensor_bytes(1, 2, "f", [0, 0, 0], vals)
    d = W.decode_node(W.encode_node(_node([dict(raw=raw)])))
    got = W.sensor_gist(d.sensors_c[0])
    assert got.tolist() == OW.float_to_byte(vals).tolist()
    assert got.tolist()[:10] == [0, 255, 255, 0, 1, 255, 0, 0, 0, 0]


def test_accessor_reports_the_count_and_respects_the_capacity():
    import ctypes as C
    raw = gist_sensor_bytes(1, 2, "f", [0, 0, 0], np.arange(40, dtype=np.float32))
    d = W.decode_node(W.encode_node(_node([dict(raw=raw)])))
    L = W._lib()
    buf = (C.c_uint8 * 8)(*([0xEE] * 8)); n = C.c_int32(-1)
    assert L.uzl_wire_sensor_gist(C.byref(d.sensors_c[0]), 5, buf, C.byref(n)) == 0
    assert n.value == 40 and list(buf) == [0, 1, 2, 3, 4, 0xEE, 0xEE, 0xEE]
    assert L.uzl_wire_sensor_gist(C.byref(d.sensors_c[0]), 5, None, C.byref(n)) == -1              # NULL output with cap > 0
    assert L.uzl_wire_sensor_gist(C.byref(d.sensors_c[0]), 0, None, None) == -1                    # NULL count
    cut = W.WireSensor(); cut.raw = W.Span(d.sensors_c[0].raw.p, len(raw) - 30)                     # ends inside the scan
    assert L.uzl_wire_sensor_gist(C.byref(cut), 0, None, C.byref(n)) == W.UZL_ERR_TRUNCATED
    small = (C.c_uint8 * 10)(); wr = C.c_uint64(0)
    g = np.zeros(32, np.uint8)
    rc = L.uzl_wire_gist_sensor_encode(0, 0, W.Span(None, 0), (C.c_double * 12)(*np.eye(3, 4).reshape(12)),
                                       g.ctypes.data_as(C.POINTER(C.c_uint8)), 32, small, 10, C.byref(wr))
    assert rc == W.UZL_ERR_TRUNCATED and wr.value == L.uzl_wire_gist_sensor_size(W.Span(None, 0), 32)


def test_gist_handle_without_gpu_fails_loudly(capi):
    if capi.device_count() > 0:
        pytest.skip("a GPU is visible")
    with pytest.raises(capi.UzlError) as e:
        capi.Gist()
    assert e.value.status == capi.UZL_ERR_NO_DEVICE
