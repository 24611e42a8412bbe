"""`utils.eval` package of the reference (utils/eval/__init__.py: `from .eval import *`): the stage-2 evaluator with the
HIP detector and NMS behind `eval.py`; the prompt generators and predicates (`lmd.py`, `utils.py`) stay the reference's
own files, reached through `__path__` when `LGD_REFERENCE_ROOT` is set."""
import os as _os

_ref = _os.environ.get("LGD_REFERENCE_ROOT")
if _ref and _os.path.isdir(_os.path.join(_ref, "utils", "eval")):
    __path__.append(_os.path.join(_ref, "utils", "eval"))   # lmd, utils: prompts and predicates

from .eval import *  # noqa: E402,F401,F403
