"""Every NS3D_* macro that a preprocessor conditional in csrc/ tests is one that some build of the library defines.

A switch that only a hand-typed -D can turn on is code no shipped build compiles and no test runs, sitting between the lines
that do the arithmetic.  The losing side of an A/B belongs in git history and its log under profiles/, not in the kernels.
Source text only: no compiler, no GPU.
"""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "navierstokes3d_amd", "csrc")

# Tested in csrc/ and defined by no build, on purpose:
ALLOWED = {
    "NS3D_PROBE": "tools/ab/resources.sh compiles one kernel instance to read its register and LDS figures",
    "NS3D_PROBE_T": "the element type of that instance",
    "NS3D_NONTEMPORAL": "ld_stream / st_stream: resolving it leaves the sweep kernels' NT parameter, a run-time variant, without meaning",
    "NS3D_NT_STORES": "the same, for the stores alone",
}

_DIRECTIVE = re.compile(r"^[ \t]*#[ \t]*(if|ifdef|ifndef|elif|else|endif|define|error)\b(.*)$")
_NAME = re.compile(r"\bNS3D_\w+")


def _directives(path):
    """(keyword, rest of the line) of every preprocessor directive, continuation lines joined, comments dropped"""
    text = open(path, encoding="utf-8").read().replace("\\\n", " ")
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    for line in text.split("\n"):
        m = _DIRECTIVE.match(line.split("//")[0])
        if m:
            yield m.group(1), m.group(2)


def _scan(path):
    """(macros tested by conditionals, macros defined on every path through the file, macros defined at all)"""
    tested, anywhere = set(), set()
    # one frame per open #if group: the macros each of its branches defines (None: the branch ends in #error), and whether it has an #else
    top = {"branches": [set()], "has_else": True}
    stack = [top]
    for kw, rest in _directives(path):
        if kw in ("if", "ifdef", "ifndef"):
            tested |= set(_NAME.findall(rest))
            stack.append({"branches": [set()], "has_else": False})
        elif kw in ("elif", "else"):
            tested |= set(_NAME.findall(rest)) if kw == "elif" else set()
            stack[-1]["branches"].append(set())
            stack[-1]["has_else"] |= kw == "else"
        elif kw == "endif":
            g = stack.pop()
            live = [b for b in g["branches"] if b is not None]
            if g["has_else"] and live and stack[-1]["branches"][-1] is not None:
                stack[-1]["branches"][-1] |= set.intersection(*live)      # defined whichever branch is taken
        elif kw == "error":
            stack[-1]["branches"][-1] = None
        elif kw == "define":
            m = _NAME.match(rest.strip())
            if m:
                anywhere.add(m.group(0))
                if stack[-1]["branches"][-1] is not None:
                    stack[-1]["branches"][-1].add(m.group(0))
    assert len(stack) == 1, "unbalanced conditionals in " + path
    return tested, top["branches"][0], anywhere


def _defined_by_builds():
    from navierstokes3d_amd import build
    out = set()
    for _src, _obj, flags in build.UNITS:
        out |= {f[2:].split("=")[0] for f in flags if f.startswith("-D")}
    assert "NS3D_MODE_STRICT" in out and "NS3D_MODE_FAST" in out      # the parser still reads the table
    return out


def test_scan_understands_branches(tmp_path):
    f = tmp_path / "x.hip"
    f.write_text("#if defined(NS3D_A) && NS3D_B > 1 // NS3D_NOT_THIS\n#define NS3D_C 1\n#elif defined(NS3D_D)\n#define NS3D_C 2\n#else\n#error \"x\"\n#endif\n"
                 "#ifndef NS3D_E\n#define NS3D_E 0   /* -DNS3D_E=1 */\n#endif\n#define NS3D_F(x) \\\n   (x)\n#if NS3D_E\n#endif\n")
    tested, always, anywhere = _scan(str(f))
    assert tested == {"NS3D_A", "NS3D_B", "NS3D_D", "NS3D_E"}
    assert always == {"NS3D_C", "NS3D_F"}           # NS3D_E only behind its own #ifndef: a -D override, not a definition
    assert anywhere == {"NS3D_C", "NS3D_E", "NS3D_F"}


def test_every_tested_switch_is_defined_by_some_build():
    headers = sorted(glob.glob(os.path.join(CSRC, "*.h"))) + [os.path.join(ROOT, "include", "ns3d.h")]
    known = _defined_by_builds()
    for h in headers:
        known |= _scan(h)[2]
    sources = sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.cpp"))) + headers
    assert len(sources) >= 7
    dead, seen, text = [], set(), ""
    for path in sources:
        tested, always, _ = _scan(path)
        seen |= tested
        text += open(path, encoding="utf-8").read()
        dead += ["%s: %s" % (os.path.basename(path), n) for n in sorted(tested - known - always - set(ALLOWED))]
    assert not dead, "conditionals on macros that no build defines (resolve them to what the library compiles):\n  " + "\n  ".join(dead)
    stale = sorted(n for n in ALLOWED if not re.search(r"\b%s\b" % n, text))
    assert not stale, "allow-list entries that the sources no longer name: %s" % stale
    assert {"NS3D_MODE_FAST", "NS3D_EXACT_RECIP", "NS3D_HAS_SLOW_PATH"} <= seen      # the scan found the kernel unit's real switches
