"""Bit-identity check between two builds of libba3c.so (A/B of a layout-only change): run as
   BA3C_LIB=<lib> python scripts/ab_bitident.py dump OUT.npz [B,B,...]   (each build, separate processes)
   python scripts/ab_bitident.py compare A.npz B.npz
dump: gradients, TfDictOp scalars, the workspace activations and every kernel's merged mask
(ba3c_kernel_merged: the launch structure) of one training pass, then the parameters after one
fused clip + Adam apply, at B=2048 (F=512, S=1), B=160 and B=32 (F=128, S=4) on fixed random
frames, or at the listed batches (B=32 at F=128, S=4; every other at F=512, S=1)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "distributed-ba3c_amd"))
sys.path.insert(0, ROOT)


def dump(out, batches=(2048, 160, 32)):
    from ba3c_amd import _lib
    from ba3c_amd.engine import Ba3cEngine
    from ba3c_amd.optimizer import AdamOptimizer
    from oracle import ba3c_oracle as O
    res = {}
    for B in batches:
        F, S = (128, 4) if B == 32 else (512, 1)
        rs = np.random.RandomState(B)
        eng = Ba3cEngine(num_actions=4, fc_neurons=F, fc_splits=S, max_batch=B)
        eng.load_params(O.init_params(F, S, 4, seed=7, dtype=np.float32))
        st = torch.from_numpy(rs.randint(0, 256, size=(B, 84, 84, 4)).astype(np.uint8)).cuda()
        ac = torch.from_numpy(rs.randint(0, 4, size=B).astype(np.int64)).cuda()
        R = torch.from_numpy(rs.normal(size=B).astype(np.float32)).cuda()
        sc = eng.train_grads(st, ac, R)
        res["B%d_grads" % B] = eng.grads.cpu().numpy()
        res["B%d_scalars" % B] = sc.cpu().numpy()
        for n in ("p1", "p2", "dp1", "dp0"):
            res["B%d_%s" % (B, n)] = eng.workspace_tensor(n, B).cpu().numpy()
        res["B%d_merged" % B] = np.array([int(eng.lib.ba3c_kernel_merged(eng.h, i))
                                          for i in sorted(_lib.KERNEL_IDS.values())], dtype=np.int64)
        AdamOptimizer(1e-3, 0.8, 0.75, 1e-8).apply_gradients(eng, fuse_clip=True)
        res["B%d_params" % B] = eng.params.cpu().numpy()
        torch.cuda.synchronize()
        assert eng.device_errors() == 0
        del eng
    np.savez(out, **res)


def compare(a, b):
    A, Bz = np.load(a), np.load(b)
    bad = [k for k in A.files if not np.array_equal(A[k], Bz[k])]
    print("bit-identical: %d of %d arrays%s" % (len(A.files) - len(bad), len(A.files),
                                                 "; differ: %s" % bad if bad else ""))
    return 0 if not bad else 1


if __name__ == "__main__":
    if sys.argv[1] == "dump":
        dump(sys.argv[2], *([[int(b) for b in sys.argv[3].split(",")]] if len(sys.argv) > 3 else []))
    else:
        sys.exit(compare(sys.argv[2], sys.argv[3]))
