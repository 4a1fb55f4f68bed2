"""Bit-identity check between two builds of libba3c.so (A/B of a layout-only change): run as
   BA3C_LIB=<lib> python scripts/ab_bitident.py dump OUT.npz [B,B,...]   (each build, separate processes)
   BA3C_LIB=<lib> python scripts/ab_bitident.py dump_ppo OUT.npz SAMPLERS.npz   (the same)
   python scripts/ab_bitident.py compare A.npz B.npz
dump: gradients, TfDictOp scalars, the workspace activations and every kernel's merged mask
(ba3c_kernel_merged: the launch structure) of one training pass, then the parameters after one
fused clip + Adam apply, at B=2048 (F=512, S=1), B=160 and B=32 (F=128, S=4) on fixed random
frames, or at the listed batches (B=32 at F=128, S=4; every other at F=512, S=1).
dump_ppo: gradient, scalars and ratio of one PPO pass through each exported entry point —
ba3c_train_grads_ppo and ba3c_train_grads_ppo_ext with vclip_eps = 0.2 and the advantage from the
row — for one configuration per heads instantiation at B=33 and (A=4, F=128, S=4) at B=260 (the
scalars' own launch), on fixed random frames and rows around the forward's own value and
log-probability; into SAMPLERS.npz ba3c_sample's actions and flag and ba3c_sample_logp's actions, logp and flag
at A in {1, 4, 18, 31} x B in {1, 100, 1000} with one row scaled by 1.01."""
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


PPO_CASES = [(33, 4, 128, 4), (33, 4, 512, 1), (33, 1, 4, 1), (33, 18, 128, 4), (33, 4, 192, 4),
             (33, 17, 500, 5), (33, 31, 516, 3), (260, 4, 128, 4)]        # (B, A, F, S)


def dump_ppo(out, out_samplers):
    from ba3c_amd import _lib
    from ba3c_amd.engine import Ba3cEngine, _ptr, _stream
    from oracle import ba3c_oracle as O
    res = {}
    for B, A, F, S in PPO_CASES:
        rs = np.random.RandomState(1000 * A + F + B)
        eng = Ba3cEngine(num_actions=A, fc_neurons=F, fc_splits=S, max_batch=B)
        eng.load_params(O.init_params(F, S, A, seed=7, dtype=np.float32))
        st = torch.from_numpy(rs.randint(0, 256, size=(B, 84, 84, 4)).astype(np.uint8)).cuda()
        ac = torch.from_numpy(rs.randint(0, A, size=B).astype(np.int64)).cuda()
        probs, _, value = (t.cpu().numpy().astype(np.float64) for t in eng.forward(st))
        lpa = np.log(probs[np.arange(B), ac.cpu().numpy()] + 1e-6)
        # ratios on both sides of the clip, values on both sides of the value clip
        rows = np.stack([value + rs.normal(size=B), value + 0.4 * rs.normal(size=B),
                         lpa + 0.3 * rs.normal(size=B), rs.normal(size=B)], axis=1).astype(np.float32)
        rw = torch.from_numpy(rows).cuda()
        ratio = torch.zeros(B, dtype=torch.float32, device="cuda")
        head = (eng.h, _stream(), _ptr(eng.params), _ptr(st), _ptr(ac), _ptr(rw), B, 0.01, 0.2)
        tail = (_ptr(eng._workspace(True)), _ptr(eng.grads), _ptr(eng.scalars), _ptr(ratio), 0)
        for leg, call in (("plain", lambda: eng.lib.ba3c_train_grads_ppo(*head, *tail)),
                          ("ext", lambda: eng.lib.ba3c_train_grads_ppo_ext(
                              *head, 0.2, _lib.PPO_ADV_FROM_ROW, *tail))):
            eng.grads.zero_()
            ratio.zero_()
            _lib.check(call())
            for n, t in (("grads", eng.grads), ("scalars", eng.scalars), ("ratio", ratio)):
                res["B%d_A%d_F%d_S%d_%s_%s" % (B, A, F, S, leg, n)] = t.cpu().numpy()
        assert eng.device_errors() == 0
        del eng
    np.savez(out, **res)
    res, eng = {}, Ba3cEngine(num_actions=4, fc_neurons=128, fc_splits=4, max_batch=16)
    for A in (1, 4, 18, 31):
        for B in (1, 100, 1000):
            rs = np.random.RandomState(A * 1000 + B)
            probs = O.softmax(rs.normal(scale=2.0, size=(B, A))).astype(np.float32)
            pi = torch.from_numpy(O.softmax(rs.normal(scale=2.0, size=(B, A))).astype(np.float32)).cuda()
            if B > 1:
                probs[B // 2] *= np.float32(1.01)
            probs, u = torch.from_numpy(probs).cuda(), torch.from_numpy(rs.random_sample(B)).cuda()
            got = eng.sample(probs, u) + eng.sample_logp(probs, pi, u)
            for n, t in zip(("a", "flag", "lp_a", "lp_logp", "lp_flag"), got):
                res["A%d_B%d_%s" % (A, B, n)] = t.cpu().numpy()
    np.savez(out_samplers, **res)


def compare(a, b):
    A, Bz = np.load(a), np.load(b)
    bad = [k for k in A.files if not np.array_equal(A[k], Bz[k])]
    print("bit-identical: %d of %d arrays%s" % (len(A.files) - len(bad), len(A.files),
                                                 "; differ: %s" % bad if bad else ""))
    return 0 if not bad else 1


if __name__ == "__main__":
    if sys.argv[1] == "dump":
        dump(sys.argv[2], *([[int(b) for b in sys.argv[3].split(",")]] if len(sys.argv) > 3 else []))
    elif sys.argv[1] == "dump_ppo":
        dump_ppo(sys.argv[2], sys.argv[3])
    else:
        sys.exit(compare(sys.argv[2], sys.argv[3]))
