"""python tests/vit_forms_child.py CASE OUT: three forwards of one case of tests/vit_forms.py in a process of its own, so that a switch C++
reads once per process (MHMR_ANYORDER: the parent sets it in this process's environment) can be compared across values.  Saves to OUT
the form bits and, for each of the three forwards, feat32 and the real rows of the fp32 residual stream."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests", "golden"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)


def main(case: str, out: str) -> int:
    import torch
    import vit_forms as vf
    from multi_hmr_amd import vit
    for k, v in vf.case_env(case).items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    P = vf.pack_case(case)
    B = vf.case_batch(case, vf.cu_count())
    cache = vit.WorkspaceCache()
    x = vf.make_images(B)
    runs = [vf.run_case(case, P, B, x, cache) for _ in range(3)]
    vf.check_want(runs[0]["bits"], vf.CASES[case]["want"], case)
    torch.save(dict(bits=sorted(runs[0]["bits"]), feat32=[r["feat32"].cpu() for r in runs],
                    resid=[r["resid"][:, :P["T"]].cpu() for r in runs]), out)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
