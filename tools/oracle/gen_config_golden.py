"""BUILD-CONTAINER ONLY: the reference's model configs (configs/gdrn/**.py), loaded unchanged through rdpn6d_amd.config.Config.fromfile
(``_base_`` chains, ``_delete_``) and stored resolved, so that the tests that build every shipped config need no reference checkout.
Keeps the sections the factory and the tests read (MODEL, SOLVER, TEST, INPUT) of every file that defines MODEL; tuples are stored as
JSON lists.  Writes tests/golden/reference_configs.json.gz.

  python tools/oracle/gen_config_golden.py <reference checkout>"""
import glob
import gzip
import json
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
sys.path.insert(0, ROOT)
from rdpn6d_amd.config import Config  # noqa: E402

SECTIONS = ("MODEL", "SOLVER", "TEST", "INPUT")


def main(ref):
    top = os.path.join(ref, "configs", "gdrn")
    out = {}
    for f in sorted(glob.glob(os.path.join(top, "**", "*.py"), recursive=True)):
        try:
            cfg = Config.fromfile(f)
        except ModuleNotFoundError:
            continue  # tlessSO/icp.py imports mmcv at module level
        if "MODEL" not in cfg:
            continue  # empty placeholder files
        out[os.path.relpath(f, top)] = {s: cfg[s] for s in SECTIONS if s in cfg}
    dst = os.path.join(ROOT, "tests", "golden", "reference_configs.json.gz")
    with gzip.GzipFile(dst, "wb", mtime=0) as g:  # (mtime 0: the same configs give the same bytes)
        g.write(json.dumps(out, sort_keys=True, separators=(",", ":")).encode())
    print(f"{len(out)} configs -> {dst}")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
