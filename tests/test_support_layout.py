"""The layering of tests/: test modules are leaves.  What several of them share -- restatements of the kernels, case
builders, harness loaders, comparison helpers -- lives in a support module (a file not named test_*), once.  Reads
import statements and function bodies only; no GPU, no library."""
import ast
import collections
import glob
import os

HERE = os.path.dirname(os.path.abspath(__file__))


def modules():
    """{file name: its syntax tree} of tests/*.py."""
    out = {}
    for path in sorted(glob.glob(os.path.join(HERE, "*.py"))):
        with open(path) as f:
            out[os.path.basename(path)] = ast.parse(f.read(), path)
    return out


def test_no_module_imports_a_test_module():
    bad = []
    for name, tree in modules().items():
        for node in ast.walk(tree):
            if isinstance(node, ast.Import):
                targets = [a.name for a in node.names]
            elif isinstance(node, ast.ImportFrom):         # the module, and what "from . import" names
                targets = [node.module or ""] + [a.name for a in node.names]
            else:
                continue
            bad += [f"{name}:{node.lineno} imports {t}" for t in targets
                    if any(part.startswith("test_") for part in t.split("."))]
    assert not bad, "\n".join(bad)


def test_no_helper_is_defined_twice():
    """No two files define a top-level non-test function with the same arguments and the same body (docstring
    ignored)."""
    where = collections.defaultdict(list)
    for name, tree in modules().items():
        for node in tree.body:
            if isinstance(node, ast.FunctionDef) and not node.name.startswith("test_"):
                body = node.body
                if body and isinstance(body[0], ast.Expr) and isinstance(body[0].value, ast.Constant) and \
                        isinstance(body[0].value.value, str):
                    body = body[1:]
                where[ast.dump(node.args), "".join(ast.dump(b) for b in body)].append(f"{name}:{node.name}")
    twice = [" == ".join(v) for v in where.values() if len({w.split(":")[0] for w in v}) > 1]
    assert not twice, "\n".join(twice)
