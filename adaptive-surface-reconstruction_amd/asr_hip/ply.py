"""Minimal PLY reader / writer for the `asrtool` command line (the reference reads its input with
cpp/bin/plyreader.h: vertex properties x, y, z, nx, ny, nz and an optional per-point radius named `value` or
`radius`, cpp/bin/main.cpp:27-112; it writes the mesh through Open3D, main.cpp:164-174)."""
import numpy as np

_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2",
          "ushort": "u2", "uint16": "u2", "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4",
          "float": "f4", "float32": "f4", "double": "f8", "float64": "f8"}


def _read_vertex_table(path):
    """-> ({property name: array [N]} of the vertex element, {property name: numpy type code})"""
    with open(path, "rb") as f:
        if f.readline().strip() != b"ply":
            raise ValueError("%s: not a PLY file" % path)
        fmt, elements = None, []
        while True:
            line = f.readline()
            if not line:
                raise ValueError("%s: truncated PLY header" % path)
            tok = line.decode("ascii", "replace").split()
            if not tok or tok[0] == "comment" or tok[0] == "obj_info":
                continue
            if tok[0] == "format":
                fmt = tok[1]
            elif tok[0] == "element":
                elements.append({"name": tok[1], "count": int(tok[2]), "props": []})
            elif tok[0] == "property":
                if tok[1] == "list":
                    elements[-1]["props"].append((tok[4], "list", tok[2], tok[3]))
                else:
                    if tok[1] not in _TYPES:
                        raise ValueError("%s: unknown property type %s" % (path, tok[1]))
                    elements[-1]["props"].append((tok[2], _TYPES[tok[1]]))
            elif tok[0] == "end_header":
                break
        if fmt not in ("ascii", "binary_little_endian", "binary_big_endian"):
            raise ValueError("%s: unsupported PLY format %r" % (path, fmt))
        data = None
        for el in elements:
            has_list = any(p[1] == "list" for p in el["props"])
            if el["name"] != "vertex":
                if has_list and fmt != "ascii":
                    raise ValueError("%s: a list element before 'vertex' cannot be skipped in a binary file" % path)
                if fmt == "ascii":
                    for _ in range(el["count"]):
                        f.readline()
                else:
                    f.seek(el["count"] * sum(np.dtype(p[1]).itemsize for p in el["props"]), 1)
                continue
            if has_list:
                raise ValueError("%s: list properties in the vertex element are not supported" % path)
            names = [p[0] for p in el["props"]]
            if fmt == "ascii":
                rows = np.loadtxt(f, dtype=np.float64, max_rows=el["count"], ndmin=2) if el["count"] else np.zeros((0, len(names)))
                data = {n: rows[:, i] for i, n in enumerate(names)}
            else:
                order = "<" if fmt == "binary_little_endian" else ">"
                dt = np.dtype([(n, order + t) for n, t in el["props"]])
                rec = np.frombuffer(f.read(dt.itemsize * el["count"]), dtype=dt, count=el["count"])
                data = {n: rec[n] for n in names}
            types = dict(el["props"])
            break
    if data is None:
        raise ValueError("%s: no vertex element" % path)
    return data, types


def read_points(path, require_normals=True):
    """-> (points f32[N,3], normals f32[N,3], radii f32[N] or f32[0]).  ValueError if a required property is
    missing (the reference returns empty arrays and then fails with "points is null!").  require_normals=False: a file
    without all of nx ny nz (a raw scan) is read too, and its normals are None."""
    data, _ = _read_vertex_table(path)
    have_normals = all(c in data for c in ("nx", "ny", "nz"))
    for req in ("x", "y", "z") + (("nx", "ny", "nz") if require_normals else ()):
        if req not in data:
            raise ValueError("%s: vertex property %s is missing (needed: x y z%s)"
                             % (path, req, " nx ny nz" if require_normals else ""))
    points = np.stack([data["x"], data["y"], data["z"]], 1).astype(np.float32)
    normals = np.stack([data["nx"], data["ny"], data["nz"]], 1).astype(np.float32) if have_normals else None
    radii = np.zeros(0, np.float32)
    for name in ("value", "radius"):  # main.cpp:103-106
        if name in data:
            radii = np.asarray(data[name], np.float32)
            break
    return points, normals, radii


def read_point_colors(path):
    """-> uint8 [N,3], the vertex properties red green blue (or diffuse_red diffuse_green diffuse_blue) of a point
    cloud, or None when the file has none.  Integer properties are taken as they are (clamped to 0..255), float
    ones as 0..1 and scaled: round(clamp(c, 0, 1) * 255)."""
    data, types = _read_vertex_table(path)
    for names in (("red", "green", "blue"), ("diffuse_red", "diffuse_green", "diffuse_blue")):
        if all(n in data for n in names):
            cols = []
            for n in names:
                c = np.asarray(data[n], np.float64)
                if types[n] in ("f4", "f8"):
                    c = np.clip(c, 0.0, 1.0) * 255.0
                cols.append(np.rint(np.clip(c, 0.0, 255.0)).astype(np.uint8))
            return np.stack(cols, 1).reshape(-1, 3)
    return None


def _check_colors(colors, n, what):
    c = np.asarray(colors)
    if c.dtype != np.uint8 or c.ndim != 2 or c.shape != (n, 3):
        raise ValueError("colors must be uint8 with one r g b row per %s" % what)
    return c


def _write_rows(f, fmt_binary, cols, colors):
    """rows of float columns followed by three uchar colour columns (when given)"""
    if colors is None:
        if fmt_binary:
            f.write(cols.astype("<f4").tobytes())
        else:
            np.savetxt(f, cols, fmt="%.9g")
        return
    if fmt_binary:
        rec = np.empty(len(cols), dtype=[("f", "<f4", (cols.shape[1],)), ("c", "u1", (3,))])
        rec["f"] = cols
        rec["c"] = colors
        f.write(rec.tobytes())
    else:
        np.savetxt(f, np.concatenate([cols.astype(np.float64), colors.astype(np.float64)], 1),
                   fmt=["%.9g"] * cols.shape[1] + ["%d"] * 3)


_COLOR_PROPS = "property uchar red\nproperty uchar green\nproperty uchar blue\n"


def write_points(path, points, normals, radii=None, binary=True, colors=None):
    """point cloud in the layout read_points takes (used by the tests and to export synthetic scans); colors
    uint8 [N,3] (optional) become the uchar properties red green blue, what read_point_colors reads"""
    points, normals = np.asarray(points, np.float32), np.asarray(normals, np.float32)
    if colors is not None:
        colors = _check_colors(colors, len(points), "point")
    cols = [points, normals] + ([np.asarray(radii, np.float32)[:, None]] if radii is not None and len(radii) else [])
    table = np.concatenate(cols, 1)
    props = ["x", "y", "z", "nx", "ny", "nz"] + (["radius"] if table.shape[1] == 7 else [])
    with open(path, "wb") as f:
        f.write(("ply\nformat %s 1.0\nelement vertex %d\n" % ("binary_little_endian" if binary else "ascii", len(table))).encode())
        f.write("".join("property float %s\n" % p for p in props).encode())
        if colors is not None:
            f.write(_COLOR_PROPS.encode())
        f.write(b"end_header\n")
        _write_rows(f, binary, table, colors)


def write_mesh(path, vertices, triangles, binary=True, normals=None, colors=None):
    """triangle mesh: vertices f32[M,3], triangles i32[T,3] (the result dict of reconstruct_surface); normals
    f32[M,3] (optional) become the vertex properties nx ny nz, colors uint8 [M,3] (optional) the uchar properties
    red green blue after them"""
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    t = np.asarray(triangles, np.int32).reshape(-1, 3)
    nprops = ""
    if colors is not None:
        colors = _check_colors(colors, len(v), "vertex")
    if normals is not None:
        nrm = np.asarray(normals, np.float32).reshape(-1, 3)
        if len(nrm) != len(v):
            raise ValueError("normals must have one row per vertex")
        v = np.concatenate([v, nrm], 1)
        nprops = "property float nx\nproperty float ny\nproperty float nz\n"
    if colors is not None:
        nprops += _COLOR_PROPS
    with open(path, "wb") as f:
        f.write(("ply\nformat %s 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n%s"
                 "element face %d\nproperty list uchar int vertex_indices\nend_header\n"
                 % ("binary_little_endian" if binary else "ascii", len(v), nprops, len(t))).encode())
        _write_rows(f, binary, v, colors)
        if binary:
            rec = np.empty(len(t), dtype=[("n", "u1"), ("i", "<i4", 3)])
            rec["n"] = 3
            rec["i"] = t
            f.write(rec.tobytes())
        else:
            np.savetxt(f, np.concatenate([np.full((len(t), 1), 3), t], 1), fmt="%d")


def read_mesh(path, with_normals=False, with_colors=False):
    """inverse of write_mesh (tests): (vertices, triangles); with_normals=True adds the normals (or None),
    with_colors=True then the uint8 [M,3] colours (or None)"""
    with open(path, "rb") as f:
        header = []
        while True:
            line = f.readline().decode("ascii").strip()
            header.append(line)
            if line == "end_header":
                break
        nv = int([h for h in header if h.startswith("element vertex")][0].split()[2])
        nt = int([h for h in header if h.startswith("element face")][0].split()[2])
        fcols = 6 if "property float nx" in header else 3
        has_colors = "property uchar red" in header
        cols = fcols + (3 if has_colors else 0)
        if "format ascii 1.0" in header:
            v = np.loadtxt(f, dtype=np.float64, max_rows=nv, ndmin=2).reshape(-1, cols)
            c = v[:, fcols:].astype(np.uint8)
            v = v[:, :fcols].astype(np.float32)
            t = np.loadtxt(f, dtype=np.int32, max_rows=nt, ndmin=2).reshape(-1, 4)[:, 1:] if nt else np.zeros((0, 3), np.int32)
        else:
            dt = np.dtype([("f", "<f4", (fcols,))] + ([("c", "u1", (3,))] if has_colors else []))
            rec = np.frombuffer(f.read(dt.itemsize * nv), dtype=dt)
            v, c = rec["f"].reshape(-1, fcols), (rec["c"].reshape(-1, 3) if has_colors else None)
            rec = np.frombuffer(f.read(13 * nt), dtype=[("n", "u1"), ("i", "<i4", 3)])
            t = rec["i"].astype(np.int32)
    v = v.astype(np.float32)
    out = (np.ascontiguousarray(v[:, :3]), t)
    if with_normals:
        out += (np.ascontiguousarray(v[:, 3:]) if fcols == 6 else None,)
    if with_colors:
        out += (np.ascontiguousarray(c) if has_colors else None,)
    return out


def average_colors(colors, vertex_map, num_out):
    """colours uint8 [V,3] of a mesh carried through the vertex_map int [V] of a simplification (-1: the vertex is
    gone): every output vertex gets the mean of the colours mapped onto it, rounded to nearest; an output vertex that
    nothing maps to is black -> uint8 [num_out,3]"""
    c = _check_colors(colors, len(vertex_map), "vertex").astype(np.float64)
    vm = np.asarray(vertex_map, np.int64)
    keep = vm >= 0
    if keep.any() and vm.max() >= num_out:
        raise ValueError("vertex_map points past the output vertices")
    total = np.zeros((num_out, 3))
    np.add.at(total, vm[keep], c[keep])
    count = np.bincount(vm[keep], minlength=num_out)[:, None]
    return np.rint(total / np.maximum(count, 1)).astype(np.uint8)


def hub_attributes(values, triangles, num_in, num_out):
    """per-vertex values [num_in,C] (normals f32 or colours uint8) of a mesh carried through a hole filling
    (ops.mesh_fill_holes): the input vertices keep theirs; every hub, a vertex >= num_in, gets the mean of the values of
    the rim vertices its new triangles (b, a, hub) name, colours rounded to nearest -> [num_out,C] of values' dtype"""
    values = np.asarray(values)
    tri = np.asarray(triangles, np.int64).reshape(-1, 3)
    fans = tri[tri[:, 2] >= num_in]
    num_hubs = num_out - num_in
    total = np.zeros((num_hubs, values.shape[1]))
    np.add.at(total, fans[:, 2] - num_in, values[fans[:, 1]].astype(np.float64))
    mean = total / np.maximum(np.bincount(fans[:, 2] - num_in, minlength=num_hubs), 1)[:, None]
    if values.dtype == np.uint8:
        mean = np.rint(mean)
    return np.concatenate([values, mean.astype(values.dtype)])


def read_surface(path):
    """A surface to compare against (asrtool --compare): -> (vertices f32 [N,3], triangles i32 [T,3] or None, normals
    f32 [N,3] or None).  A file with a non-empty face element is a triangle mesh in the layout write_mesh produces; one
    without faces is a point cloud, whose nx ny nz are returned when present."""
    faces = 0
    with open(path, "rb") as f:
        if f.readline().strip() != b"ply":
            raise ValueError("%s: not a PLY file" % path)
        for line in f:
            tok = line.decode("ascii", "replace").split()
            if tok[:2] == ["element", "face"]:
                faces = int(tok[2])
            if tok[:1] == ["end_header"]:
                break
    if faces > 0:
        v, t, n = read_mesh(path, with_normals=True)
        return v, t, n
    data, _ = _read_vertex_table(path)
    for req in ("x", "y", "z"):
        if req not in data:
            raise ValueError("%s: vertex property %s is missing" % (path, req))
    points = np.stack([data["x"], data["y"], data["z"]], 1).astype(np.float32)
    normals = None
    if all(k in data for k in ("nx", "ny", "nz")):
        normals = np.stack([data["nx"], data["ny"], data["nz"]], 1).astype(np.float32)
    return points, None, normals
