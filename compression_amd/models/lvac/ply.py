"""A small PLY 1.0 reader and writer for voxelised point clouds (what models/lvac/lvac.ipynb uses the `plyfile` package
for): `ascii` and `binary_little_endian`, a `vertex` element with scalar x, y, z and red, green, blue properties of any
scalar type.  Everything else in the file (comments, other vertex properties, later elements such as faces) is carried
through byte for byte; a layout that cannot be placed is a ValueError that says so."""
from __future__ import annotations

import numpy as np

__all__ = ["read_plyfile", "create_new_plyfile"]

SCALAR_TYPES = {
    "char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2",
    "uint16": "u2", "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4",
    "double": "f8", "float64": "f8"}
POSITION = ("x", "y", "z")
COLOUR = ("red", "green", "blue")


class _Layout:
    """The header of a file, and where its vertex data lies."""

    def __init__(self, blob, filename):
        self.blob = blob
        end = blob.find(b"end_header")
        newline = blob.find(b"\n", end) if end >= 0 else -1
        if not blob.startswith(b"ply") or end < 0 or newline < 0:
            raise ValueError(f"{filename}: not a PLY file (no 'ply' ... 'end_header' header)")
        self.body = newline + 1
        self.format = None
        self.elements = []                 # [name, count, [(property name, type or None for a list)]]
        for raw in blob[:end].decode("ascii", "replace").splitlines()[1:]:
            words = raw.split()
            if not words or words[0] in ("comment", "obj_info"):
                continue
            if words[0] == "format":
                if len(words) != 3 or words[2] != "1.0":
                    raise ValueError(f"{filename}: unsupported PLY version in {raw!r} (1.0 is supported)")
                if words[1] not in ("ascii", "binary_little_endian"):
                    raise ValueError(f"{filename}: unsupported PLY format {words[1]!r} (ascii and "
                                     "binary_little_endian are supported)")
                self.format = words[1]
            elif words[0] == "element" and len(words) == 3:
                self.elements.append([words[1], int(words[2]), []])
            elif words[0] == "property" and self.elements:
                if words[1] == "list":
                    self.elements[-1][2].append((words[-1], None))
                elif len(words) == 3 and words[1] in SCALAR_TYPES:
                    self.elements[-1][2].append((words[2], SCALAR_TYPES[words[1]]))
                else:
                    raise ValueError(f"{filename}: unsupported property line {raw!r}")
            else:
                raise ValueError(f"{filename}: unsupported header line {raw!r}")
        if self.format is None:
            raise ValueError(f"{filename}: the header has no format line")
        names = [e[0] for e in self.elements]
        if "vertex" not in names:
            raise ValueError(f"{filename}: the file has no vertex element")
        at = names.index("vertex")
        self.before = self.elements[:at]
        _, self.count, self.properties = self.elements[at]
        if any(t is None for _, t in self.properties):
            raise ValueError(f"{filename}: unsupported layout: the vertex element has a list property")
        self.names = [n for n, _ in self.properties]
        if self.format == "binary_little_endian":
            skip = 0
            for name, count, props in self.before:
                if any(t is None for _, t in props):
                    raise ValueError(f"{filename}: unsupported layout: element {name!r} with a list property lies "
                                     "in front of the vertex data")
                skip += count * sum(np.dtype(t).itemsize for _, t in props)
            self.dtype = np.dtype([(n, "<" + t) for n, t in self.properties])
            self.start = self.body + skip
            self.stop = self.start + self.count * self.dtype.itemsize
            if self.stop > len(blob):
                raise ValueError(f"{filename}: the file ends inside the vertex data")
        else:
            # one line per row of every element
            lines_before = sum(count for _, count, _ in self.before)
            at = self.body
            for _ in range(lines_before):
                at = self._next_line(at, filename)
            self.start = at
            for _ in range(self.count):
                at = self._next_line(at, filename)
            self.stop = at

    def _next_line(self, at, filename):
        nl = self.blob.find(b"\n", at)
        if nl < 0:
            if at < len(self.blob):
                return len(self.blob)
            raise ValueError(f"{filename}: the file ends inside the vertex data")
        return nl + 1

    def rows(self):
        """The vertex rows as a list of token lists (ascii) or a structured array (binary)."""
        if self.format == "binary_little_endian":
            return np.frombuffer(self.blob, self.dtype, self.count, self.start).copy()
        lines = self.blob[self.start:self.stop].decode("ascii").splitlines()
        rows = [line.split() for line in lines]
        if any(len(r) != len(self.properties) for r in rows):
            raise ValueError("a vertex line does not have one value per property")
        return rows

    def column(self, rows, name):
        k = self.names.index(name)
        t = np.dtype(self.properties[k][1])
        if self.format == "binary_little_endian":
            return rows[name].astype(t)
        return np.array([float(r[k]) if t.kind == "f" else int(r[k]) for r in rows], dtype=t)


def _load(filename):
    with open(filename, "rb") as f:
        return _Layout(f.read(), filename)


def read_plyfile(filename):
    """-> (position [N, 3], colour [N, 3]) in the file's own scalar types; either is None if the vertex element lacks
    x, y, z or red, green, blue."""
    layout = _load(filename)
    rows = layout.rows()

    def take(names):
        if not all(n in layout.names for n in names):
            return None
        return np.stack([layout.column(rows, n) for n in names], axis=-1)

    return take(POSITION), take(COLOUR)


def _as_type(values, t):
    """Colours as the property's type: integers are rounded to nearest and kept inside the type's range."""
    t = np.dtype(t)
    values = np.asarray(values, dtype=np.float64)
    if t.kind in "iu":
        info = np.iinfo(t)
        values = np.clip(np.rint(values), info.min, info.max)
    return values.astype(t)


def create_new_plyfile(old_filename, new_filename, colors):
    """Writes a copy of `old_filename` with the vertex colours replaced by colors [N, 3]; every other byte is kept."""
    layout = _load(old_filename)
    colors = np.asarray(colors)
    if colors.shape != (layout.count, 3):
        raise ValueError(f"colors must be [{layout.count}, 3], received shape {colors.shape}")
    if not all(n in layout.names for n in COLOUR):
        raise ValueError(f"{old_filename}: the vertex element has no red, green, blue properties")
    rows = layout.rows()
    if layout.format == "binary_little_endian":
        for j, name in enumerate(COLOUR):
            rows[name] = _as_type(colors[:, j], layout.dtype[name])
        data = rows.tobytes()
    else:
        for j, name in enumerate(COLOUR):
            k = layout.names.index(name)
            t = np.dtype(layout.properties[k][1])
            column = _as_type(colors[:, j], t)
            for row, v in zip(rows, column):
                row[k] = repr(float(v)) if t.kind == "f" else str(int(v))
        data = "".join(" ".join(row) + "\n" for row in rows).encode("ascii")
    with open(new_filename, "wb") as f:
        f.write(layout.blob[:layout.start])
        f.write(data)
        f.write(layout.blob[layout.stop:])
