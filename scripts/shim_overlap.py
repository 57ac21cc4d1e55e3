"""How much of shim/Optimizer_hip.cpp is textually the reference's cslam/src/Optimizer.cpp (CPU; needs the reference tree).

Both files are stripped of comments and of ALL whitespace; lines of 6 characters or fewer and lines that are only braces, `else`, `continue;`, `break;`
or `return;` are dropped.  Printed: how many of the shim's remaining lines occur verbatim among the reference's, per function of the shim and in total, against the
number of the shim's non-blank code lines.

    shim_overlap.py [reference root, default /root/reference] [shim file]"""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRIVIAL = re.compile(r"^([{}();]*|else|continue;|break;|return;|[{}]*else[{}]*)$")


def code_lines(text):
    text = re.sub(r"/\*.*?\*/", lambda m: "\n" * m.group(0).count("\n"), text, flags=re.S)
    out = []
    for raw in text.split("\n"):
        line = re.sub(r"\s+", "", re.sub(r"//.*", "", raw))
        out.append(line)
    return out


def counts(line):
    return len(line) > 6 and not TRIVIAL.match(line)


def function_of_lines(raw_lines):
    """name of the function a line belongs to: the last line at brace depth <= 1 (inside namespaces) that opened a body and names something callable"""
    names, cur = [], "elsewhere"
    for raw in raw_lines:
        m = re.match(r"^(?:template\s*<[^>]*>\s*)?[A-Za-z_][\w:<>\*&, ]*?\b((?:Optimizer::)?[A-Za-z_]\w*)\s*\([^;]*$", raw)
        if m and not raw.startswith((" ", "\t", "#", "//")) and m.group(1) not in ("if", "for", "while", "switch"):
            cur = m.group(1)
        elif re.match(r"^(struct|class)\s+(\w+)", raw):
            cur = re.match(r"^(struct|class)\s+(\w+)", raw).group(2)
        elif raw.startswith("}"):
            names.append(cur)
            cur = "elsewhere"
            continue
        names.append(cur)
    return names


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    shim = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "shim", "Optimizer_hip.cpp")
    ref = os.path.join(ref_root, "cslam", "src", "Optimizer.cpp")
    if not os.path.exists(ref):
        print(f"shim_overlap: {ref} is not present: nothing to compare")
        return 0
    ref_set = {l for l in code_lines(open(ref, errors="replace").read()) if counts(l)}
    text = open(shim).read()
    lines, owner = code_lines(text), function_of_lines(text.split("\n"))
    per = {}
    for l, fn in zip(lines, owner):
        if counts(l):
            t = per.setdefault(fn, [0, 0])
            t[0] += l in ref_set
            t[1] += 1
    non_blank = sum(1 for l in lines if l)
    for fn, (s, n) in sorted(per.items(), key=lambda kv: -kv[1][0]):
        if s:
            print(f"{fn:40s} {s:4d} of {n:4d}")
    shared, total = sum(v[0] for v in per.values()), sum(v[1] for v in per.values())
    print(f"{'total':40s} {shared:4d} of {non_blank:4d} non-blank code lines occur verbatim in Optimizer.cpp ({100.0 * shared / non_blank:.1f} %); "
          f"{total} lines are left after dropping the trivial ones")
    return 0


if __name__ == "__main__":
    sys.exit(main())
