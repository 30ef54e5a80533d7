#!/usr/bin/env python3
"""Writes tests/golden/conv1x1_pipeline.pt: the LDS-weight 1x1 kernel's outputs for BIT_CASES of
tests/test_gpu_conv1x1_pipeline.py (exact digests of every case, a few tensors whole).  Run on the GPU at the commit
whose numerics are the contract (the parent of a change to the kernel's main loop); the test then holds every later
build to those bits.  usage: python3 tools/gen_conv1x1_pipeline_golden.py [out.pt]"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), ROOT, os.path.join(ROOT, "neural-pde-surrogates_amd")):
    sys.path.insert(0, p)

import test_gpu_conv1x1_pipeline as t  # noqa: E402

out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "conv1x1_pipeline.pt")
gold = {"digest": {}, "full": {}}
for name in t.BIT_CASES:
    r = t.run(name)
    err = (torch.linalg.vector_norm(r["y"].double() - r["ref"]) / torch.linalg.vector_norm(r["ref"])).item()
    assert err < t.TOL, (name, err)  # a fixture of wrong outputs would pin them
    gold["digest"][name] = t.digest(r["y"])
    if name in t.BIT_FULL:
        gold["full"][name] = r["y"].clone()
    print(f"{name}: {tuple(r['y'].shape)} rel-L2 vs fp64 {err:.2e}")
torch.save(gold, out)
print(f"wrote {out}: {os.path.getsize(out)} bytes")
