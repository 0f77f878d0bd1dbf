"""tests/golden/superpoint_state_dict_keys.json: the state_dict key names and shapes of the reference's OWN SuperPoint module (superpoint.ipynb cell 1,
`SuperPointNet`, executed from the notebook at run time -- nothing is copied into the repo), in the module's order.  tests/test_weights_cpu.py holds the
.pth loader to it where the reference tree is absent.

Run from the repo root:  python tests/golden/make_golden_sp_keys.py <reference tree>/d2frontend/superpoint.ipynb
"""
import json, os, sys
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
NB = sys.argv[1]
cells = ["".join(c["source"]) for c in json.load(open(NB))["cells"]]
ns = {"torch": torch}
exec(compile(cells[1], NB + ":cell1", "exec"), ns)
sd = ns["SuperPointNet"]().state_dict()
json.dump({"module": "SuperPointNet (d2frontend/superpoint.ipynb, cell 1)", "keys": list(sd), "shapes": {k: list(v.shape) for k, v in sd.items()}},
          open(os.path.join(HERE, "superpoint_state_dict_keys.json"), "w"))
