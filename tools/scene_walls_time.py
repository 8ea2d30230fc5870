#!/usr/bin/env python3
"""ms per gym.simulate() (2 sub-steps) of the test arm's scene on the HIP backend, protocol of tools/scene_time.py (30 calls to warm up, 100 timed, one
synchronisation at the end; three repeats, each printed):

    python tools/scene_walls_time.py SCENE [num_envs ...]        SCENE: two (a slab and a wall: capacity 4) | pen (eight walls and a slab: capacity 12)

MI_SCENE_LANES=4|8 forces the envs per workgroup; MI_TREE=<dir> times another checkout of the package (an A/B against the parent commit: the scene
`two` needs nothing this tree adds).  The robot and the scene builder are those of tests/test_scene_shapes.py."""
import os
import sys
import time

ROOT = os.path.abspath(os.environ.get("MI_TREE") or os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from test_scene_shapes import I4, SLAB_T, TOP, _quat, _scene  # noqa: E402

EDGE, CX, CY, APO, WALL_T, WALL_H = 0.05, 0.5, 0.0, 0.2, 0.04, 0.12


def statics_of(scene):
    slab = ((0.6, 0.6, SLAB_T), (CX, CY, 1.0), I4)
    hw = (APO + WALL_T) * np.tan(np.pi / 8)
    wall = lambda k: ((WALL_T, 2 * hw, WALL_H), (CX + (APO + WALL_T / 2) * np.cos(np.pi * k / 4), CY + (APO + WALL_T / 2) * np.sin(np.pi * k / 4),  # noqa: E731
                                                 TOP + WALL_H / 2 - 0.02), _quat([0, 0, 1], np.pi * k / 4))
    return [wall(0), slab] if scene == "two" else [wall(k) for k in range(8)] + [slab]


def main():
    scene = sys.argv[1]
    for n in [int(a) for a in sys.argv[2:]] or [4096]:
        st = statics_of(scene)
        gym, sim, arm, root = _scene("cuda:0", st, [("box", (EDGE,) * 3, (CX, CY, TOP + EDGE / 2), I4)], n=n)
        # every env: the cube 1 cm in front of wall 0, sliding into it at 0.5 m/s -- it rests on the slab against the wall (8 contacts) from then on
        a = 1 + len(st)
        root[:, a, 0] = CX + APO - EDGE / 2 - 0.01
        root[:, a, 7] = 0.5
        ids = (torch.arange(n, device=root.device, dtype=torch.int32) * root.shape[1] + a).contiguous()
        gym.set_actor_root_state_tensor_indexed(sim, root.view(-1, 13), ids, len(ids))
        for _ in range(30):
            gym.simulate(sim)
        torch.cuda.synchronize()
        ms = []
        for _ in range(3):
            t = time.perf_counter()
            for _ in range(100):
                gym.simulate(sim)
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t) / 100 * 1e3)
        nc = sim.engine.tensors["scene_contacts"]
        cap = sim.engine.get_option("scene_static_capacity") if not os.environ.get("MI_TREE") else 4
        print(f"scene {scene}@{n} capacity {int(cap)} lanes {os.environ.get('MI_SCENE_LANES', 'default')} tree {os.path.basename(ROOT)}: "
              f"{' / '.join(f'{m:.3f}' for m in ms)} ms per gym.simulate(); contacts per env {float(nc[:, 0].float().mean()):.1f}, refused {int(nc[:, 1].sum())}", flush=True)


if __name__ == "__main__":
    main()
