"""CPU tests (no GPU): SensorData.depth_image.color on the wire - uzl_wire_sensor_color reads the colour image of a DepthImage
SensorData (bgr8, or rgb8 whose channels are swapped on upload) into what uzl_cloud_add_images takes.  The messages are built with
struct from SensorData.msg and sensor_msgs/Image by the helpers of tests/test_laserline_wire.py and go through oracle/wire.py's node
encoder."""
import ctypes as C

import numpy as np
import pytest

import oracle.wire as OW
import test_laserline_wire as TLW
from uzliti_slam_amd import capi, wire as W


def color_image(encoding, pad=0, h=3, w=4, seed=0):
    px = np.random.default_rng(seed).integers(0, 256, (h, w, 3)).astype(np.uint8)
    rows = [px[r].tobytes() + bytes(range(1, pad + 1)) for r in range(h)]
    return dict(seq=4, stamp_sec=1400000003, stamp_nsec=78, frame_id="camera_rgb_optical_frame", height=h, width=w, encoding=encoding,
                is_bigendian=0, step=3 * w + pad, data=b"".join(rows)), px


def sensor(color_bytes):
    im, _ = TLW._depth("32FC1", np.random.default_rng(1))
    raw = TLW.depth_sensor_bytes(1400000003, 77, "camera_depth_optical_frame", [0.1, 0.0, 0.3], im, color_bytes, TLW.camera_info_bytes(640, 480, TLW.P))
    node = TLW._node([dict(raw=raw)])
    assert OW.encode_node(node) == W.encode_node(node)                       # the oracle's encoder writes the same message
    return raw, W.decode_node(OW.encode_node(node))


@pytest.mark.parametrize("encoding,pad,code", [("bgr8", 0, capi.COLOR_BGR8), ("rgb8", 0, capi.COLOR_RGB8), ("bgr8", 5, capi.COLOR_BGR8)])
def test_decode(encoding, pad, code):
    im, px = color_image(encoding, pad)
    raw, d = sensor(TLW.image_bytes(im))
    out = capi.ColorImage()
    assert capi.lib().uzl_wire_sensor_color(C.byref(d.sensors_c[0]), C.byref(out)) == 0
    assert (out.width, out.height, out.step, out.encoding) == (4, 3, 12 + pad, code)
    assert C.string_at(out.data, 2 * out.step + 12) == im["data"][:2 * out.step + 12]
    got = np.frombuffer(C.string_at(out.data, 3 * out.step), np.uint8).reshape(3, out.step)[:, :12].reshape(3, 4, 3)
    assert np.array_equal(got, px)
    # the data is borrowed from the message, not copied
    base = d.sensors_c[0].raw.p
    assert base <= out.data < base + d.sensors_c[0].raw.n


def test_other_encodings_are_unsupported():
    for enc in ("mono8", "bgra8", "rgb16", "BGR8", ""):
        im, _ = color_image(enc)
        _, d = sensor(TLW.image_bytes(im))
        out = capi.ColorImage()
        assert capi.lib().uzl_wire_sensor_color(C.byref(d.sensors_c[0]), C.byref(out)) == W.UZL_ERR_UNSUPPORTED, enc


def test_the_default_image_is_unsupported_and_null_arguments_are_refused():
    _, d = sensor(None)                                                      # default-constructed colour image: empty encoding
    out = capi.ColorImage()
    L = capi.lib()
    assert L.uzl_wire_sensor_color(C.byref(d.sensors_c[0]), C.byref(out)) == W.UZL_ERR_UNSUPPORTED
    assert L.uzl_wire_sensor_color(None, C.byref(out)) == -1 and L.uzl_wire_sensor_color(C.byref(d.sensors_c[0]), None) == -1
    im, _ = color_image("bgr8", h=0, w=0)
    _, d = sensor(TLW.image_bytes(im))
    assert L.uzl_wire_sensor_color(C.byref(d.sensors_c[0]), C.byref(out)) == 0 and (out.width, out.height, out.data) == (0, 0, None)


def test_truncation_at_every_byte():
    """a sensor cut anywhere before the end of its colour image is UZL_ERR_TRUNCATED, never a read past the end"""
    im, _ = color_image("bgr8", 2)
    color = TLW.image_bytes(im)
    raw, d = sensor(color)
    out = capi.ColorImage()
    assert raw.index(color) + len(color) < len(raw)
    for n in range(len(raw)):
        w = W.WireSensor(); w.raw = W.Span(d.sensors_c[0].raw.p, n)
        assert capi.lib().uzl_wire_sensor_color(C.byref(w), C.byref(out)) == W.UZL_ERR_TRUNCATED, n
    w = d.sensors_c[0]
    assert capi.lib().uzl_wire_sensor_color(C.byref(w), C.byref(out)) == 0


def test_a_short_data_array_or_step_is_truncated():
    im, _ = color_image("bgr8")
    for bad in (dict(step=11), dict(data=im["data"][:-1]), dict(height=4)):
        _, d = sensor(TLW.image_bytes(dict(im, **bad)))
        out = capi.ColorImage()
        assert capi.lib().uzl_wire_sensor_color(C.byref(d.sensors_c[0]), C.byref(out)) == W.UZL_ERR_TRUNCATED, bad
