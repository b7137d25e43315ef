"""Minimal PLY vertex I/O (binary little-endian / ascii) for GaussianRenderer.save_ply / load_ply
(core/gs.py:101-190, which uses the external `plyfile`, absent here). Writes exactly what plyfile writes for a
single 'vertex' element of float32 properties, so files interoperate with 3DGS viewers and gui.py.
write_mesh_ply / read_mesh_ply: a triangle mesh (vertex + face elements) for lgm_amd.mesh."""
from __future__ import annotations

import numpy as np

_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2",
          "ushort": "u2", "uint16": "u2", "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4",
          "float": "f4", "float32": "f4", "double": "f8", "float64": "f8"}


def write_ply(path: str, names, data: np.ndarray) -> None:
    data = np.ascontiguousarray(data, dtype="<f4")
    assert data.ndim == 2 and data.shape[1] == len(names)
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {data.shape[0]}"]
    header += [f"property float {n}" for n in names]
    header += ["end_header"]
    with open(path, "wb") as f:
        f.write(("\n".join(header) + "\n").encode("ascii"))
        f.write(data.tobytes())


def write_mesh_ply(path: str, vertices: np.ndarray, faces: np.ndarray, colors: np.ndarray = None) -> None:
    """A triangle mesh as binary little-endian PLY: a vertex element (float x y z, and uchar red green blue when
    colors [Nv, 3] in [0, 1] are given) and a face element (`list uchar int vertex_indices`), the layout mesh viewers
    and plyfile read."""
    vertices = np.ascontiguousarray(vertices, dtype="<f4").reshape(-1, 3)
    faces = np.ascontiguousarray(faces, dtype="<i4").reshape(-1, 3)
    props = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {len(vertices)}",
              "property float x", "property float y", "property float z"]
    if colors is not None:
        colors = np.asarray(colors, dtype=np.float64).reshape(-1, 3)
        assert len(colors) == len(vertices)
        props += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
        header += ["property uchar red", "property uchar green", "property uchar blue"]
    header += [f"element face {len(faces)}", "property list uchar int vertex_indices", "end_header"]
    vrec = np.empty(len(vertices), dtype=np.dtype(props))
    vrec["x"], vrec["y"], vrec["z"] = vertices[:, 0], vertices[:, 1], vertices[:, 2]
    if colors is not None:
        c8 = np.clip(np.rint(np.nan_to_num(colors) * 255.0), 0, 255).astype(np.uint8)
        vrec["red"], vrec["green"], vrec["blue"] = c8[:, 0], c8[:, 1], c8[:, 2]
    frec = np.empty(len(faces), dtype=np.dtype([("n", "u1"), ("v", "<i4", (3,))]))
    frec["n"], frec["v"] = 3, faces
    with open(path, "wb") as f:
        f.write(("\n".join(header) + "\n").encode("ascii"))
        f.write(vrec.tobytes())
        f.write(frec.tobytes())


def read_mesh_ply(path: str):
    """Reads what write_mesh_ply wrote: (vertices [Nv, 3] float32, faces [Nf, 3] int32, colors [Nv, 3] uint8 or None)."""
    with open(path, "rb") as f:
        if f.readline().strip() != b"ply":
            raise ValueError(f"{path}: not a PLY file")
        nv = nf = 0
        vprops = []
        cur = None
        while True:
            line = f.readline()
            if not line:
                raise ValueError(f"{path}: truncated header")
            tok = line.decode("ascii").strip().split()
            if not tok:
                continue
            if tok[0] == "format" and tok[1] != "binary_little_endian":
                raise ValueError(f"{path}: {tok[1]} is not supported")
            if tok[0] == "element":
                cur = tok[1]
                if cur == "vertex":
                    nv = int(tok[2])
                elif cur == "face":
                    nf = int(tok[2])
            elif tok[0] == "property" and cur == "vertex":
                vprops.append((tok[2], "<" + _TYPES[tok[1]] if _TYPES[tok[1]][1] != "1" else _TYPES[tok[1]]))
            elif tok[0] == "property" and cur == "face" and tok[1:4] != ["list", "uchar", "int"]:
                raise ValueError(f"{path}: face property {' '.join(tok[1:])} is not supported")
            elif tok[0] == "end_header":
                break
        vdt = np.dtype(vprops)
        vrec = np.frombuffer(f.read(vdt.itemsize * nv), dtype=vdt, count=nv)
        fdt = np.dtype([("n", "u1"), ("v", "<i4", (3,))])
        frec = np.frombuffer(f.read(fdt.itemsize * nf), dtype=fdt, count=nf)
    if nf and not (frec["n"] == 3).all():
        raise ValueError(f"{path}: only triangles are supported")
    vertices = np.stack([vrec["x"], vrec["y"], vrec["z"]], axis=1).astype(np.float32)
    colors = np.stack([vrec["red"], vrec["green"], vrec["blue"]], axis=1) if "red" in vdt.names else None
    return vertices, np.array(frec["v"], dtype=np.int32).reshape(-1, 3), colors


def read_ply(path: str) -> dict:
    """Returns {property name: 1-D numpy array} of the first element (vertices)."""
    with open(path, "rb") as f:
        if f.readline().strip() != b"ply":
            raise ValueError(f"{path}: not a PLY file")
        fmt, elements, cur = None, [], None
        while True:
            line = f.readline()
            if not line:
                raise ValueError(f"{path}: truncated header")
            tok = line.decode("ascii").strip().split()
            if not tok:
                continue
            if tok[0] == "format":
                fmt = tok[1]
            elif tok[0] == "element":
                cur = [tok[1], int(tok[2]), []]
                elements.append(cur)
            elif tok[0] == "property":
                if tok[1] == "list":
                    raise ValueError("list properties are not supported")
                cur[2].append((tok[2], _TYPES[tok[1]]))
            elif tok[0] == "end_header":
                break
        name, count, props = elements[0]
        if fmt == "ascii":
            rows = [f.readline().decode("ascii").split() for _ in range(count)]
            arr = np.array(rows, dtype=np.float64).reshape(count, len(props))
            return {p[0]: arr[:, i].astype(p[1]) for i, p in enumerate(props)}
        endian = "<" if fmt == "binary_little_endian" else ">"
        dt = np.dtype([(p[0], endian + p[1]) for p in props])
        rec = np.frombuffer(f.read(dt.itemsize * count), dtype=dt, count=count)
        return {p[0]: np.asarray(rec[p[0]]).astype(p[1].replace(">", "<")) for p in props}
