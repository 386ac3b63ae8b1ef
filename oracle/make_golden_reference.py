"""Fixtures for the two tests that used to read the live reference tree (build container only; writes data, never source):

  * tests/golden/reference_config.json -- the defaults of the reference's ThermalNerfactoModelConfig, field by field (camera optimiser configs:
    their plain fields), which tests/test_host_cpu.py compares this package's configuration mirror with;
  * tests/golden/hash_encoding.npz -- one case of the reference's HashEncoding(implementation="torch"): its table, the query points and its
    output, which tests/test_oracle_vs_golden.py compares the oracle's hash encoding with, bit for bit.

Imports the reference through oracle/ref_import.py.  Runs on the CPU in seconds:  python oracle/make_golden_reference.py"""
import dataclasses
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(os.path.dirname(HERE), "tests", "golden")
sys.path.insert(0, HERE)

import ref_import  # noqa: E402


def _plain(v):
    if isinstance(v, (tuple, list)):
        return [_plain(x) for x in v]
    if isinstance(v, dict):
        return {k: _plain(x) for k, x in v.items()}
    return v


def config_defaults():
    from nerfstudio.models.thermal_nerfacto import ThermalNerfactoModelConfig as RefCfg

    ref = RefCfg()
    out = {}
    for f in dataclasses.fields(ref):
        if f.name in ("_target", "implementation"):  # (the class itself; "tcnn"/"torch" there, the HIP library here)
            continue
        b = getattr(ref, f.name)
        if dataclasses.is_dataclass(b):  # camera optimizer configs: the plain fields
            out[f.name] = {"dataclass": {g.name: _plain(getattr(b, g.name)) for g in dataclasses.fields(b) if g.name not in ("_target", "optimizer", "scheduler")}}
        else:
            out[f.name] = {"value": _plain(b)}
    return out


def hash_encoding_case():
    from nerfstudio.field_components.encodings import HashEncoding

    torch.manual_seed(0)
    enc = HashEncoding(num_levels=5, min_res=16, max_res=256, log2_hashmap_size=10, implementation="torch")
    x = torch.rand(1000, 3)
    with torch.no_grad():
        out = enc(x)
    return {"hash_table": enc.hash_table.detach().numpy(), "x": x.numpy(), "out": out.numpy(), "num_levels": 5, "min_res": 16, "max_res": 256,
            "log2_hashmap_size": 10}


if __name__ == "__main__":
    ref_import.import_reference()
    cfg = config_defaults()
    with open(os.path.join(GOLDEN, "reference_config.json"), "w") as f:
        json.dump(cfg, f, indent=1, sort_keys=True)
    np.savez_compressed(os.path.join(GOLDEN, "hash_encoding.npz"), **hash_encoding_case())
    print(f"{len(cfg)} config fields, hash encoding case written under {GOLDEN}")
