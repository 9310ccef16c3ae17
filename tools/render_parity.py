#!/usr/bin/env python3
"""Depth parity of the frame renderer (csrc/qa_render.hip) against the float64 reference tests/render_ref.py, on the GPU: for every scene of
cases 1-3 of tests/test_render.py (single primitives over the plane at 64 x 48 and 61 x 35, the engine-posed robots, the tilted height
field with its block, the ceiling with its hole, the map's border) the maximum of |fp32 - float64| / max(1, depth) over the pixels that are
not edge pixels, the share of edge pixels, and the share of pixels whose 8-bit colour differs by one level.  tests/test_render.py holds
its depth bound to 4 x the largest maximum written here.

  python tools/render_parity.py [--out profiles/render_parity.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_parity.json"))
    args = ap.parse_args()
    import numpy as np
    from tests import render_ref as rr
    from tests import render_scenes as rs
    from tests import test_render as tr
    scenes = dict(analytic=rs.attach(rs.analytic_scene()), analytic_61x35=rs.attach(rs.analytic_scene(61, 35)), engine=tr.engine_scene(),
                  heightfield=rs.attach(rs.heightfield_scene()), ceiling=rs.attach(rs.ceiling_scene()), border=rs.attach(rs.border_scene()))
    out = {"metric": "max over off-edge pixels of |depth_fp32 - depth_float64| / max(1, depth_float64)", "scenes": {}}
    for name, scene in scenes.items():
        ids, depth, rgb = tr.gpu_render(scene)
        rows = []
        for k in range(len(scene["env_ids"])):
            rid, rdepth, rrgb, edge = rr.render(scene, k)
            ok = ~edge
            rel = np.abs(depth[k] - rdepth) / np.maximum(1.0, rdepth)
            diff = np.abs(rgb[k].astype(np.int64) - rrgb.astype(np.int64)).max(axis=-1)
            rows.append(dict(camera=k, edge_share=float(edge.mean()), ids_differing_off_edge=int((ok & (ids[k] != rid)).sum()),
                             depth_rel_err_max=float(rel[ok].max()), rgb_off_by_one_share=float((diff[ok] == 1).mean()),
                             rgb_off_by_more=int((diff[ok] > 1).sum())))
        out["scenes"][name] = dict(width=scene["width"], height=scene["height"], cameras=rows,
                                   depth_rel_err_max=max(r["depth_rel_err_max"] for r in rows))
        print(name, json.dumps(out["scenes"][name]["cameras"]))
    out["depth_rel_err_max"] = max(s["depth_rel_err_max"] for s in out["scenes"].values())
    out["test_bound"] = 4 * out["depth_rel_err_max"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("largest:", out["depth_rel_err_max"], "->", args.out)


if __name__ == "__main__":
    main()
