#!/usr/bin/env python3
"""Depth parity of the course mode of the frame renderer (csrc/qa_render_course.hip) against the float64 reference
tests/render_course_ref.py, on the GPU: for every scene of tests/render_course_scenes.py (the see-saw at both stops and between, bar and tyre
at 96 x 64 and 61 x 35, the goals, the static map) the maximum of |fp32 - float64| / max(1, depth) over the pixels that are not edge pixels,
the share of edge pixels, and the share of pixels whose 8-bit colour differs by one level.  tests/test_render_course.py holds its depth
bound to 4 x the larger of tests/test_render.py's measured value and the largest maximum written here.

  python tools/render_course_parity.py [--out profiles/render_course_parity.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_course_parity.json"))
    args = ap.parse_args()
    import numpy as np
    from tests import render_course_scenes as cs
    from tests import test_render as tr
    from tests import test_render_course as trc
    out = {"metric": "max over off-edge pixels of |depth_fp32 - depth_float64| / max(1, depth_float64)", "scenes": {}}
    for name in sorted(cs.SCENES):
        scene = cs.scene(name)
        ids, depth, rgb = trc.gpu_render(scene)
        rows = []
        for k in range(len(scene["env_ids"])):
            rid, rdepth, rrgb, edge = cs.reference(name, k)
            ok = ~edge
            rel = np.abs(depth[k] - rdepth) / np.maximum(1.0, rdepth)
            diff = np.abs(rgb[k].astype(np.int64) - rrgb.astype(np.int64)).max(axis=-1)
            rows.append(dict(camera=k, edge_share=float(edge.mean()), ids_differing_off_edge=int((ok & (ids[k] != rid)).sum()),
                             depth_rel_err_max=float(rel[ok].max()), rgb_off_by_one_share=float((diff[ok] == 1).mean()),
                             rgb_off_by_more=int((diff[ok] > 1).sum()), ids=sorted(set(rid.ravel().tolist()))))
        out["scenes"][name] = dict(width=scene["width"], height=scene["height"], cameras=rows, depth_rel_err_max=max(r["depth_rel_err_max"] for r in rows))
        print(name, json.dumps(out["scenes"][name]["cameras"]))
    out["depth_rel_err_max"] = max(s["depth_rel_err_max"] for s in out["scenes"].values())
    out["test_render_measured"] = tr.DEPTH_REL_MEASURED
    out["test_bound"] = 4 * max(out["depth_rel_err_max"], tr.DEPTH_REL_MEASURED)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("largest:", out["depth_rel_err_max"], "->", args.out)


if __name__ == "__main__":
    main()
