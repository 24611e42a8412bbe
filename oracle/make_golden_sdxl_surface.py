"""Golden module surface of the reference's generation/sdxl_refinement.py (BASELINE config 5): its module-level
string constants and the parameters (with defaults) of its functions, read with `ast` from the reference's own,
unmodified file — nothing of it is imported or executed.

    python oracle/make_golden_sdxl_surface.py REFERENCE_ROOT   # writes tests/golden/sdxl_refinement_surface.json

Needs a checkout of the reference; the JSON is committed and checked by
tests/test_sdxl_cpu.py::test_dropin_module_surface_matches_the_reference."""
import ast
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))

tree = ast.parse(open(os.path.join(sys.argv[1], "generation", "sdxl_refinement.py")).read())
constants = {n.targets[0].id: n.value.value for n in tree.body
             if isinstance(n, ast.Assign) and isinstance(n.value, ast.Constant) and isinstance(n.value.value, str)}
functions = {}
for n in tree.body:
    if isinstance(n, ast.FunctionDef):
        params = [a.arg for a in n.args.args]
        defaults = [ast.literal_eval(d) for d in n.args.defaults]
        functions[n.name] = dict(params=params, defaults=dict(zip(params[len(params) - len(defaults):], defaults)))
out = os.path.join(HERE, "..", "tests", "golden", "sdxl_refinement_surface.json")
json.dump(dict(source="generation/sdxl_refinement.py", constants=constants, functions=functions), open(out, "w"), indent=1)
print("wrote", out)
