#!/usr/bin/env python3
"""Generates jittor-myc-nerfs_amd/csrc/tvr_mc_table.h: the marching-cubes case table of csrc/tvr_mesh.hip, built by construction.

    python scripts/gen_mc_table.py            # rewrites the committed header
    python scripts/gen_mc_table.py --check    # exit status 1 if the committed header differs

Conventions
  * corner c of a cell has offset (c & 1, (c >> 1) & 1, (c >> 2) & 1) in (x, y, z); bit c of a case index is set iff corner c is INSIDE (value >= level);
  * edge e = 4 * axis + n joins the n-th corner (ascending) whose `axis` bit is clear to the corner with that bit set: EDGE_CORNERS below.  The edge's owner
    is the grid point of its lower corner, and `axis` is e >> 2.

Construction, per case
  1. on each of the six faces the cut edges are joined by the marching-squares rule; on a face with four cut edges every INSIDE corner is cut off on its own.
     The rule reads only the face's four flags, so the two cells that share a face draw the same segments on it;
  2. every segment is directed so that the surface normal (right-hand rule) points from inside to outside: seen from outside the cell, the inside corners lie to
     the right of the direction of travel, i.e. (d x m) . n > 0 for direction d, face normal n and the in-face vector m from the inside to the outside corners;
  3. every cut edge then has one segment arriving and one leaving: the segments form closed directed loops;
  4. each loop is triangulated as a fan; loops are ordered by their lowest-numbered edge.  The fan's apex is the lowest-numbered edge of the loop from which no
     diagonal of the fan lies inside a face of the cell.  (A diagonal inside a face joins two cut edges of a four-cut face; the neighbouring cell, which draws
     the same segments on that face, can lay a diagonal of its own on the same two edges, and that mesh edge would then carry four triangles.  With the plain
     "lowest-numbered edge" apex 18 loops of 6 or 7 edges have such a diagonal under this edge numbering; every loop has an apex without one.)
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "jittor-myc-nerfs_amd", "csrc", "tvr_mc_table.h")
MAX_TRIS = 5

CORNERS = np.array([[c & 1, (c >> 1) & 1, (c >> 2) & 1] for c in range(8)], dtype=np.int64)
EDGE_CORNERS = [(lo, lo | (1 << axis)) for axis in range(3) for lo in range(8) if not lo & (1 << axis)]        # 12 x (lower corner, upper corner)
EDGE_OF = {frozenset(ec): e for e, ec in enumerate(EDGE_CORNERS)}
EDGE_MID = np.array([(CORNERS[a] + CORNERS[b]) / 2.0 for a, b in EDGE_CORNERS])
# face (axis, side): its four corners, and its outward normal
FACES = [(axis, side, [c for c in range(8) if ((c >> axis) & 1) == side]) for axis in range(3) for side in (0, 1)]


def face_normal(axis: int, side: int) -> np.ndarray:
    n = np.zeros(3)
    n[axis] = 1.0 if side else -1.0
    return n


def face_edges(corners) -> list:
    """The four cell edges that lie in a face."""
    return [EDGE_OF[frozenset((a, b))] for i, a in enumerate(corners) for b in corners[i + 1:] if frozenset((a, b)) in EDGE_OF]


def face_segments(case: int, axis: int, side: int, corners) -> list:
    """Directed marching-squares segments [(edge from, edge to)] of one face under the face rule."""
    inside = [c for c in corners if (case >> c) & 1]
    outside = [c for c in corners if not (case >> c) & 1]
    cut = [e for e in face_edges(corners) if ((case >> EDGE_CORNERS[e][0]) & 1) != ((case >> EDGE_CORNERS[e][1]) & 1)]
    if not cut:
        return []
    n = face_normal(axis, side)
    centre = CORNERS[corners].mean(0)
    pairs = []           # (two edges, vector from the inside to the outside of the segment)
    if len(cut) == 2:
        pairs.append((cut, CORNERS[outside].mean(0) - CORNERS[inside].mean(0)))
    else:                # four cut edges: the two inside corners are diagonal; each is cut off on its own
        assert len(cut) == 4 and len(inside) == 2
        for c in inside:
            pairs.append(([e for e in cut if c in EDGE_CORNERS[e]], centre - CORNERS[c]))
    out = []
    for (e0, e1), m in pairs:
        d = EDGE_MID[e1] - EDGE_MID[e0]
        s = float(np.dot(np.cross(d, m), n))
        assert abs(s) > 1e-9
        out.append((e0, e1) if s > 0 else (e1, e0))
    return out


def case_loops(case: int) -> list:
    nxt = {}
    for axis, side, corners in FACES:
        for a, b in face_segments(case, axis, side, corners):
            assert a not in nxt, "a cut edge has two segments leaving it"
            nxt[a] = b
    assert sorted(nxt) == sorted(set(nxt.values())), "a cut edge lacks an arriving or a leaving segment"
    loops, seen = [], set()
    for start in sorted(nxt):
        if start in seen:
            continue
        loop, e = [], start
        while e not in seen:
            seen.add(e)
            loop.append(e)
            e = nxt[e]
        assert e == start and len(loop) >= 3
        loops.append(loop)            # starts at its lowest-numbered edge: `start` ascends
    return loops


def share_face(e0: int, e1: int) -> bool:
    both = set(EDGE_CORNERS[e0]) | set(EDGE_CORNERS[e1])
    return any(both <= set(corners) for _, _, corners in FACES)


def fan(loop) -> list:
    """Triangles of a loop: a fan from the lowest-numbered edge none of whose diagonals lies inside a face."""
    n = len(loop)
    for apex in sorted(loop):
        r = loop[loop.index(apex):] + loop[:loop.index(apex)]
        if not any(share_face(r[0], r[i]) for i in range(2, n - 1)):
            return [(r[0], r[i], r[i + 1]) for i in range(1, n - 1)]
    raise AssertionError("no fan of this loop avoids the faces")


def case_triangles(case: int) -> list:
    return [t for loop in case_loops(case) for t in fan(loop)]


def build_table():
    """(tri [256, MAX_TRIS, 3] int8 padded with -1, count [256] uint8)"""
    tri = np.full((256, MAX_TRIS, 3), -1, dtype=np.int8)
    cnt = np.zeros(256, dtype=np.uint8)
    for case in range(256):
        t = case_triangles(case)
        assert len(t) <= MAX_TRIS
        cnt[case] = len(t)
        if t:
            tri[case, :len(t)] = t
    return tri, cnt


def header_text() -> str:
    tri, cnt = build_table()
    L = ["// tvr_mc_table.h — GENERATED by scripts/gen_mc_table.py; do not edit (tests/test_mesh_host.py compares it with the generator's output).",
         "// Marching-cubes case table of tvr_mesh.hip.  Corner c of a cell sits at offset (c & 1, (c >> 1) & 1, (c >> 2) & 1) in (x, y, z); bit c of a case is set iff",
         "// value >= level there.  Edge e runs along axis e >> 2 from corner TVR_MC_EDGE_LO[e] (its owner point) to that corner with the axis bit set.",
         f"// {int(cnt.sum())} triangles over the 256 cases, at most {int(cnt.max())} per case; normals (right-hand rule) point from inside to outside.",
         "#pragma once",
         "",
         f"#define TVR_MC_MAX_TRIS {MAX_TRIS}",
         "",
         "static __device__ const unsigned char TVR_MC_EDGE_LO[12] = {" + ", ".join(str(lo) for lo, _ in EDGE_CORNERS) + "};",
         "",
         "// triangles per case",
         "static __device__ const unsigned char TVR_MC_TRI_COUNT[256] = {"]
    for r in range(0, 256, 32):
        L.append("    " + ", ".join(str(int(x)) for x in cnt[r:r + 32]) + ",")
    L += ["};", "", "// edge numbers of the triangles of each case, in emission order; 255 pads the unused slots",
          "static __device__ const unsigned char TVR_MC_TRI[256][3 * TVR_MC_MAX_TRIS] = {"]
    for case in range(256):
        row = ", ".join(f"{int(x) & 255:3d}" for x in tri[case].reshape(-1))
        L.append(f"    {{{row}}},   // {case}")
    L += ["};", ""]
    return "\n".join(L)


def main(argv) -> int:
    text = header_text()
    if "--check" in argv:
        same = os.path.exists(HEADER) and open(HEADER).read() == text
        print("tvr_mc_table.h is up to date" if same else "tvr_mc_table.h differs from the generator's output")
        return 0 if same else 1
    with open(HEADER, "w") as f:
        f.write(text)
    tri, cnt = build_table()
    print(f"wrote {HEADER}: {int(cnt.sum())} triangles, at most {int(cnt.max())} per case")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
