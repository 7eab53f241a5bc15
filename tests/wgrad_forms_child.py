"""Child of test_wgrad_forms_gpu.py::test_environment_selected_forms: the tuning switches of kpf_conv2d_wgrad are read once per process, so each setting gets a
process of its own.  Runs lin, k3 and trim in both 16-bit types with nothing forced (the canary checks of wgrad_forms.run included) and prints one line
"WGRAD_CHILD <json>": per case the family the plan query names and (e_kernel, e_plain) of dw and db.  The parent applies the bound."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import wgrad_forms as WF  # noqa: E402


def main():
    rows = []
    for kind in ("bf16", "f16"):
        for name in ("lin", "k3", "trim"):
            v = WF.variant(name, kind)
            dw, db, p = WF.run(v, 0)
            e = WF.errors(v, dw, db)
            rows.append({"variant": name, "kind": kind, "family": WF.family(p), "S": p.S, "dw": e["dw"], "db": e["db"]})
    print("WGRAD_CHILD " + json.dumps(rows))


if __name__ == "__main__":
    main()
