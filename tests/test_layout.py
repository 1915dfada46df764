"""CPU: the layout rule of tests/ (tests/README.md): shared test code lives in support modules, never in a test file.  No
tests/test_*.py imports from a module named test_*, and no support module defines a test."""
import ast
import glob
import os

HERE = os.path.dirname(os.path.abspath(__file__))


def _trees(pattern):
    return [(os.path.basename(f), ast.parse(open(f).read(), f)) for f in sorted(glob.glob(os.path.join(HERE, pattern)))]


def test_no_test_file_imports_another_and_no_support_module_defines_a_test():
    tests = _trees("test_*.py")
    assert len(tests) > 40  # the glob found the suite
    for name, tree in tests:
        for node in ast.walk(tree):
            if isinstance(node, ast.Import):
                mods = [a.name for a in node.names]
            elif isinstance(node, ast.ImportFrom):
                mods = [node.module or ""] + [f"{node.module or ''}.{a.name}" for a in node.names]
            else:
                continue
            for m in mods:
                assert not m.split(".")[-1].startswith("test_"), f"{name}:{node.lineno} imports {m}"
    support = [(n, t) for n, t in _trees("*.py") if not n.startswith("test_")]
    assert {"gpu_support.py", "gpu_cases.py", "oracle_support.py", "abi_support.py"} <= {n for n, _ in support}
    for name, tree in support:
        for node in ast.walk(tree):
            if isinstance(node, (ast.FunctionDef, ast.AsyncFunctionDef)):
                assert not node.name.startswith("test_"), f"{name}:{node.lineno} defines {node.name}"
