"""Child of test_dw7_forms_gpu.py::test_switch_selected_forms: the tuning switches of the depthwise 7x7 family are read once per process, so each setting gets a
process of its own.  argv[1] names the cases the setting bears on: "fwd" (kpf_dwconv7_f32 / _add_f32 on the training shapes), "wgrad" (kpf_dwconv7_wgrad on its
shapes), "ln_wave" / "ln_wide" (kpf_dwconv7_ln_* on the shapes the lane-group / the wide kernel takes by default, every storage type).  Nothing is forced: the
cases run as the dispatcher sends them under the environment, with the guard checks of dw7_forms, and one line "DW7_CHILD <json>" carries per comparison the
plan the query names, the figures of the bound and a CRC of the output's bits.  The parent checks that the switch was seen and applies the bounds."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import dw7_forms as DF  # noqa: E402


def _plan(p):
    return {"family": DF.family(p), "form": DF.form(p), "px": p.px, "rows": p.rows, "taps_lds": p.taps_lds, "S": p.S, "rows_per_chunk": p.rows_per_chunk,
            "cq": p.cq, "raise_lds": p.raise_lds}


def main(group):
    rows = []
    if group == "fwd":
        for name in DF.TRAIN_CASES:
            v = DF.train_case(name)
            for op in ("fwd", "dgrad", "dgrad_add"):
                y, p = DF.run_conv(name, op)
                ek, ep = DF.rel_errors(y, v.ref[op], v.plain[op])
                rows.append({"op": op, "case": name, "kind": "f32", "plan": _plan(p), "fig": {"e_kernel": ek, "e_plain": ep}, "crc": DF.crc(y)})
    elif group == "wgrad":
        for name in DF.WGRAD_CASES:
            v = DF.train_case(name)
            dw, db, p = DF.run_wgrad(name)
            for what, got in (("dw", dw), ("db", db)):
                ek, ep = DF.rel_errors(got, v.ref[what], v.plain[what])
                rows.append({"op": what, "case": name, "kind": "f32", "plan": _plan(p), "fig": {"e_kernel": ek, "e_plain": ep}, "crc": DF.crc(got)})
    else:
        for name in DF.LN_CASES:
            if not name.startswith(group[3:]):
                continue
            for kind in DF.ln_kinds(name):
                y, p = DF.run_ln(name, kind)
                rows.append({"op": "ln", "case": name, "kind": kind, "plan": _plan(p), "fig": DF.ln_figures(DF.ln_case(name, kind), kind, y), "crc": DF.crc(y)})
    print("DW7_CHILD " + json.dumps(rows))


if __name__ == "__main__":
    main(sys.argv[1])
