"""PLY reader and writer for the reference's initialisation files, with no plyfile / open3d dependency.

``read_ply`` returns what the reference reads of such a file (``plydata.elements[0][name]``, gstex.py:608-694): the
scalar properties of the file's FIRST element, one 1-D array per property in the file's own type.  Elements after the
first (a mesh's ``face`` with its list property, say) are not parsed.  ``write_ply`` writes one element of scalar
columns, little-endian binary or ascii.  ``write_mesh_ply`` writes a triangle mesh: a ``vertex`` element and a
``face`` element with the usual ``vertex_indices`` list.

Sizes come from the header and are checked against the file's length before any array is made; nothing is read past
the first element's rows.  Every defect is a ``PlyError`` naming the path.
"""
from __future__ import annotations

import itertools
import os

import numpy as np

# PLY type name -> numpy type code (without byte order); both spellings of the format
_TYPES = {
    "char": "i1", "uchar": "u1", "short": "i2", "ushort": "u2", "int": "i4", "uint": "u4", "float": "f4",
    "double": "f8",
    "int8": "i1", "uint8": "u1", "int16": "i2", "uint16": "u2", "int32": "i4", "uint32": "u4", "float32": "f4",
    "float64": "f8",
}
_NAMES = {"i1": "char", "u1": "uchar", "i2": "short", "u2": "ushort", "i4": "int", "u4": "uint", "f4": "float",
          "f8": "double"}
_FORMATS = {"ascii": None, "binary_little_endian": "<", "binary_big_endian": ">"}
_MAX_HEADER = 1 << 20  # bytes; a 2DGS header with 62 properties has about 1.5 kB


class PlyError(ValueError):
    """A file that is not the PLY its header (or its caller) says it is."""


def _read_header(f, path):
    """(format, element name, row count, [(property name, type code)], data offset) of the first element."""
    first = f.readline(_MAX_HEADER)
    if first.rstrip(b"\r\n") != b"ply":
        raise PlyError(f"{path}: not a PLY file (the first line is not 'ply')")
    fmt = None
    elements = []  # [name, count, properties]; only the first element's properties are parsed
    while True:
        raw = f.readline(_MAX_HEADER)
        if not raw or f.tell() > _MAX_HEADER:
            raise PlyError(f"{path}: no end_header line" + ("" if not raw else f" in the first {_MAX_HEADER} bytes"))
        try:
            line = raw.decode("ascii").strip()
        except UnicodeDecodeError:
            raise PlyError(f"{path}: the header is not ascii (no end_header line before the data?)") from None
        words = line.split()
        if not words:
            continue
        key = words[0]
        if key == "end_header":
            break
        if key in ("comment", "obj_info"):
            continue
        if key == "format":
            if len(words) != 3 or words[1] not in _FORMATS:
                raise PlyError(f"{path}: unknown format line {line!r} (ascii, binary_little_endian or "
                               "binary_big_endian)")
            fmt = words[1]
        elif key == "element":
            if len(words) != 3 or not words[2].isdigit():
                raise PlyError(f"{path}: bad element line {line!r}")
            elements.append([words[1], int(words[2]), []])
        elif key == "property":
            if not elements:
                raise PlyError(f"{path}: property line {line!r} before any element")
            if len(elements) > 1:
                continue  # not ours: later elements are never read
            if len(words) >= 2 and words[1] == "list":
                raise PlyError(f"{path}: list property {words[-1]!r} in the first element "
                               f"({elements[0][0]!r}); only scalar properties can be read")
            if len(words) != 3:
                raise PlyError(f"{path}: bad property line {line!r}")
            if words[1] not in _TYPES:
                raise PlyError(f"{path}: unknown type {words[1]!r} of property {words[2]!r}")
            if any(words[2] == name for name, _ in elements[0][2]):
                raise PlyError(f"{path}: property {words[2]!r} is declared twice")
            elements[0][2].append((words[2], _TYPES[words[1]]))
        else:
            raise PlyError(f"{path}: unknown header line {line!r} (no end_header line before the data?)")
    if fmt is None:
        raise PlyError(f"{path}: no format line")
    if not elements:
        raise PlyError(f"{path}: no element")
    name, count, props = elements[0]
    return fmt, name, count, props, f.tell()


def _ascii_column(tokens, code, path, name):
    try:
        if code[0] == "f":
            return np.array([float(t) for t in tokens], dtype=code)
        values = [int(t) for t in tokens]
    except ValueError:
        raise PlyError(f"{path}: property {name!r} has a value that is no {_NAMES[code]}") from None
    info = np.iinfo(code)
    if values and (min(values) < info.min or max(values) > info.max):
        raise PlyError(f"{path}: property {name!r} has a value outside the range of {_NAMES[code]}")
    return np.array(values, dtype=code)


def read_ply(path) -> dict:
    """{property name: 1-D array} of the first element's scalar properties, in file order, each in the file's own
    type (native byte order)."""
    path = os.fspath(path)
    with open(path, "rb") as f:
        fmt, element, count, props, offset = _read_header(f, path)
        left = os.fstat(f.fileno()).st_size - offset
        order = _FORMATS[fmt]
        if order is not None:
            row = np.dtype([(f"f{i}", order + code) for i, (_, code) in enumerate(props)]) if props else None
            need = count * (row.itemsize if props else 0)
            if need > left:
                raise PlyError(f"{path}: truncated: the header promises {count} {element} rows of "
                               f"{row.itemsize} bytes ({need} bytes), the file holds {left}")
            if not props:
                return {}
            data = np.fromfile(f, dtype=row, count=count)
            if data.shape[0] != count:  # (the file shrank under us)
                raise PlyError(f"{path}: truncated: read {data.shape[0]} of {count} {element} rows")
            return {name: np.ascontiguousarray(data[f"f{i}"]).astype(code) for i, (name, code) in enumerate(props)}
        # ascii: a row is at least one character and one separator per value
        if count * 2 * len(props) > left + 1:
            raise PlyError(f"{path}: truncated: the header promises {count} {element} rows of {len(props)} values, "
                           f"the file holds {left} bytes of data")
        rows = []
        for raw in itertools.islice(f, count):
            words = raw.split()
            if len(words) != len(props):
                raise PlyError(f"{path}: {element} row {len(rows)} has {len(words)} values, the header declares "
                               f"{len(props)}")
            rows.append(words)
        if len(rows) != count:
            raise PlyError(f"{path}: truncated: the header promises {count} {element} rows, the file holds "
                           f"{len(rows)}")
        return {name: _ascii_column([r[i].decode("ascii", "replace") for r in rows], code, path, name)
                for i, (name, code) in enumerate(props)}


def write_mesh_ply(path, vertices, faces, colors=None) -> None:
    """A triangle mesh, little-endian binary: a `vertex` element of float x, y, z and, with `colors` (V, 3) in [0, 1],
    uchar red, green, blue = clamp(c, 0, 1) * 255 truncated; then a `face` element of `property list uchar int
    vertex_indices`, three indices per face.  read_ply of the file returns the vertex columns."""
    path = os.fspath(path)
    v = np.ascontiguousarray(np.asarray(vertices, dtype=np.float32))
    f = np.ascontiguousarray(np.asarray(faces))
    if v.ndim != 2 or v.shape[1] != 3:
        raise PlyError(f"{path}: vertices have shape {v.shape}; expected (V, 3)")
    if f.size == 0:
        f = f.reshape(0, 3)
    if f.ndim != 2 or f.shape[1] != 3 or f.dtype.kind not in "iu":
        raise PlyError(f"{path}: faces have shape {f.shape} and dtype {f.dtype}; expected integer (F, 3)")
    if f.size and (int(f.min()) < 0 or int(f.max()) >= v.shape[0]):
        raise PlyError(f"{path}: a face index is outside [0, {v.shape[0]})")
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    if colors is not None:
        c = np.asarray(colors, dtype=np.float32)
        if c.shape != v.shape:
            raise PlyError(f"{path}: colors have shape {c.shape}, vertices {v.shape}")
        rgb = (np.clip(c, np.float32(0.0), np.float32(1.0)) * np.float32(255.0)).astype(np.uint8)
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
    vdata = np.empty(v.shape[0], dtype=fields)
    for k, name in enumerate("xyz"):
        vdata[name] = v[:, k]
    if colors is not None:
        for k, name in enumerate(("red", "green", "blue")):
            vdata[name] = rgb[:, k]
    fdata = np.empty(f.shape[0], dtype=[("n", "u1"), ("i", "<i4", (3,))])
    fdata["n"] = 3
    fdata["i"] = f
    head = ["ply", "format binary_little_endian 1.0", f"element vertex {v.shape[0]}"]
    head += [f"property {_NAMES[code.lstrip('<')]} {name}" for name, code in fields]
    head += [f"element face {f.shape[0]}", "property list uchar int vertex_indices", "end_header"]
    with open(path, "wb") as out:
        out.write(("\n".join(head) + "\n").encode("ascii"))
        vdata.tofile(out)
        fdata.tofile(out)


def write_ply(path, columns, *, binary: bool = True, element: str = "vertex", comments=()) -> None:
    """One element of scalar properties: `columns` maps property names to equal-length 1-D arrays whose dtypes
    (int8 .. uint32, float32, float64) give the PLY types.  binary: little-endian; else ascii, floats with the digits
    that read back exactly."""
    path = os.fspath(path)
    cols = []
    for name, values in columns.items():
        a = np.asarray(values)
        code = a.dtype.kind + str(a.dtype.itemsize)
        if code not in _NAMES:
            raise PlyError(f"{path}: column {name!r} has dtype {a.dtype}, which PLY has no scalar type for")
        if a.ndim != 1:
            raise PlyError(f"{path}: column {name!r} has shape {a.shape}; columns are 1-D")
        if not isinstance(name, str) or not name or len(name.split()) != 1:
            raise PlyError(f"{path}: {name!r} is no property name")
        cols.append((name, code, a))
    n = cols[0][2].shape[0] if cols else 0
    for name, _, a in cols:
        if a.shape[0] != n:
            raise PlyError(f"{path}: column {name!r} has {a.shape[0]} rows, {cols[0][0]!r} has {n}")
    if len(element.split()) != 1:
        raise PlyError(f"{path}: {element!r} is no element name")
    head = ["ply", f"format {'binary_little_endian' if binary else 'ascii'} 1.0"]
    for c in comments:
        if "\n" in c or "\r" in c:
            raise PlyError(f"{path}: a comment spans lines")
        head.append(f"comment {c}")
    head.append(f"element {element} {n}")
    head += [f"property {_NAMES[code]} {name}" for name, code, _ in cols]
    head.append("end_header")
    with open(path, "wb") as f:
        f.write(("\n".join(head) + "\n").encode("ascii"))
        if binary:
            if cols:
                data = np.empty(n, dtype=[(f"f{i}", "<" + code) for i, (_, code, _) in enumerate(cols)])
                for i, (_, _, a) in enumerate(cols):
                    data[f"f{i}"] = a
                data.tofile(f)
            return
        text = [[repr(float(v)) for v in a] if code[0] == "f" else [str(int(v)) for v in a] for _, code, a in cols]
        for r in range(n):
            f.write((" ".join(t[r] for t in text) + "\n").encode("ascii"))
