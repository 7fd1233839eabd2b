"""gstex_amd.ply: the PLY reader and writer behind the initialisation files.  CPU only."""
import numpy as np
import pytest

from gstex_amd.ply import PlyError, read_ply, write_ply

# a hand-written file (not made by write_ply): mixed types, both spellings, comments, a trailing face element
ASCII_PLY = """ply
format ascii 1.0
comment made by hand
obj_info nothing to see
element vertex 3
property float x
property double y
property uchar red
property int16 id
property uint32 big
property char tiny
comment a comment between properties
element face 2
property list uchar int vertex_indices
end_header
0.5 -1.25 255 -300 4294967295 -128
1e-3 2.0 0 7 0 127
-3 0.1 17 32767 12 0
3 0 1 2
3 2 1 0
"""

TYPES = ["int8", "uint8", "int16", "uint16", "int32", "uint32", "float32", "float64"]


def _write(tmp_path, text, name="a.ply", newline="\n"):
    path = tmp_path / name
    path.write_bytes(text.replace("\n", newline).encode("ascii") if isinstance(text, str) else text)
    return path


def _check_literal(cols):
    assert list(cols) == ["x", "y", "red", "id", "big", "tiny"]
    expect = {"x": np.array([0.5, 1e-3, -3], np.float32), "y": np.array([-1.25, 2.0, 0.1], np.float64),
              "red": np.array([255, 0, 17], np.uint8), "id": np.array([-300, 7, 32767], np.int16),
              "big": np.array([4294967295, 0, 12], np.uint32), "tiny": np.array([-128, 127, 0], np.int8)}
    for k, v in expect.items():
        assert cols[k].dtype == v.dtype and cols[k].shape == (3,), k
        assert np.array_equal(cols[k], v), k


def test_literal_ascii_file_with_a_trailing_face_element(tmp_path):
    _check_literal(read_ply(_write(tmp_path, ASCII_PLY)))


def test_crlf_header_lines(tmp_path):
    _check_literal(read_ply(_write(tmp_path, ASCII_PLY, newline="\r\n")))


def _columns(n=37, seed=0):
    rng = np.random.default_rng(seed)
    cols = {}
    for t in TYPES:
        dt = np.dtype(t)
        if dt.kind == "f":
            a = rng.normal(0, 1, n).astype(dt) * dt.type(10.0) ** rng.integers(-30, 30, n).astype(dt)
            a[:4] = [0.1, -0.0, np.finfo(dt).max, np.finfo(dt).tiny]
        else:
            info = np.iinfo(dt)
            a = rng.integers(info.min, info.max, n, dtype=dt, endpoint=True)
            a[:2] = [info.min, info.max]
        cols[f"c_{t}"] = a
    return cols


@pytest.mark.parametrize("binary", [True, False])
def test_round_trip_is_exact_for_every_type(tmp_path, binary):
    cols = _columns()
    path = tmp_path / "rt.ply"
    write_ply(path, cols, binary=binary, element="splat", comments=("one", "two"))
    head = path.read_bytes().split(b"end_header\n")[0].decode("ascii").splitlines()
    assert head[:4] == ["ply", f"format {'binary_little_endian' if binary else 'ascii'} 1.0", "comment one",
                        "comment two"]
    assert head[4] == "element splat 37"
    assert head[5:] == ["property char c_int8", "property uchar c_uint8", "property short c_int16",
                        "property ushort c_uint16", "property int c_int32", "property uint c_uint32",
                        "property float c_float32", "property double c_float64"]
    back = read_ply(path)
    assert list(back) == list(cols)
    for k, v in cols.items():
        assert back[k].dtype == v.dtype, k
        assert back[k].tobytes() == v.tobytes(), k  # bit-equal (-0.0 included)


def test_big_endian_file(tmp_path):
    n = 5
    x = np.arange(n, dtype=np.float32) * 1.5 - 2
    i = np.array([-70000, 1, 2, 3, 2**31 - 1], np.int32)
    d = np.linspace(-1, 1, n)
    h = np.array([1, 2, 3, 60000, 5], np.uint16)
    data = np.empty(n, dtype=[("x", ">f4"), ("i", ">i4"), ("d", ">f8"), ("h", ">u2")])
    data["x"], data["i"], data["d"], data["h"] = x, i, d, h
    head = ("ply\nformat binary_big_endian 1.0\nelement vertex 5\nproperty float x\nproperty int i\n"
            "property double d\nproperty ushort h\nend_header\n")
    cols = read_ply(_write(tmp_path, head.encode("ascii") + data.tobytes() + b"trailing bytes are not read"))
    for k, v in (("x", x), ("i", i), ("d", d), ("h", h)):
        assert cols[k].dtype == v.dtype and cols[k].dtype.isnative and np.array_equal(cols[k], v), k


def test_empty_element(tmp_path):
    path = tmp_path / "e.ply"
    write_ply(path, {"x": np.zeros(0, np.float32)})
    cols = read_ply(path)
    assert list(cols) == ["x"] and cols["x"].shape == (0,) and cols["x"].dtype == np.float32


HEAD = "ply\nformat {fmt} 1.0\nelement vertex {n}\nproperty float x\nproperty {t} y\nend_header\n"


@pytest.mark.parametrize("text, what", [
    ("plx\nformat ascii 1.0\nelement vertex 0\nend_header\n", "not a PLY"),
    ("ply\nformat ascii 1.0\nelement vertex 1\nproperty float x\n1.0\n", "end_header"),
    (HEAD.format(fmt="binary_middle_endian", n=1, t="float") + "xxxxxxxx", "format"),
    (HEAD.format(fmt="ascii", n=1, t="half") + "1 2\n", "unknown type"),
    ("ply\nformat ascii 1.0\nelement vertex 1\nproperty list uchar int idx\nend_header\n1 0\n", "list property"),
    (HEAD.format(fmt="ascii", n=3, t="float") + "1 2\n3 4\n", "truncated"),       # fewer rows
    (HEAD.format(fmt="ascii", n=2, t="float") + "1 2\n3\n5 6\n", "values"),       # fewer columns in a row
    (HEAD.format(fmt="ascii", n=1, t="uchar") + "1 256\n", "range"),
    (HEAD.format(fmt="ascii", n=1, t="int") + "1 1.5\n", "no int"),
    (HEAD.format(fmt="binary_little_endian", n=2, t="float") + "x" * 15, "truncated"),
])
def test_rejections(tmp_path, text, what):
    path = _write(tmp_path, text)
    with pytest.raises(PlyError, match=what) as e:
        read_ply(path)
    assert str(path) in str(e.value)
    assert isinstance(e.value, ValueError)


def test_truncated_binary_raises_before_allocating(tmp_path, monkeypatch):
    """A header that promises 2^40 rows over 8 data bytes: refused from the file's length, before any array of the
    header's size is asked for (np.fromfile / np.empty are made to fail the test if reached)."""
    path = _write(tmp_path, HEAD.format(fmt="binary_little_endian", n=2**40, t="double") + "x" * 8)

    def boom(*a, **k):
        raise AssertionError("allocated from the header's count")

    monkeypatch.setattr(np, "fromfile", boom)
    monkeypatch.setattr(np, "empty", boom)
    monkeypatch.setattr(np, "zeros", boom)
    with pytest.raises(PlyError, match="truncated"):
        read_ply(path)
    # the ascii branch has the same guard
    path = _write(tmp_path, HEAD.format(fmt="ascii", n=2**40, t="double") + "1 2\n", name="b.ply")
    with pytest.raises(PlyError, match="truncated"):
        read_ply(path)


def test_writer_refuses_what_ply_cannot_hold(tmp_path):
    for cols in ({"x": np.zeros(3, np.int64)}, {"x": np.zeros((3, 1), np.float32)},
                 {"x": np.zeros(3, np.float32), "y": np.zeros(2, np.float32)}, {"a b": np.zeros(3, np.float32)}):
        with pytest.raises(PlyError):
            write_ply(tmp_path / "w.ply", cols)
