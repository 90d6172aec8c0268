"""Builds tests/golden/reference_tree_facts.json: what tests/test_rust_identifiers.py and
tests/test_integration_artifacts.py need to know about the reference tree, so that they run without it.

    python tests/golden/make_reference_tree_facts.py <path of the reference tree>

Two kinds of facts, data only:

  * `rust_index`: the names the reference's src/**/*.rs define (tests/rust_index.py: functions with their arities, items,
    struct fields, enum variants, the functions of each type's impl blocks), restricted to the identifiers the Rust side of
    integration/ actually uses -- every lookup the identifier test makes is on such a name -- plus the sizes of the whole
    index.  A new name in the patches is `unknown` until this file is rebuilt.
  * `patch_base`: for every file integration/lorikeet-hip.patch touches, whether the reference has it, its line count, and
    the SHA-256 of the reference's lines under each hunk of the patch (`-start,count` of the hunk header).  A hunk whose
    pre-image hashes to that value applies at the line it names: what `git apply --check` verifies against the tree.
Rebuild it whenever either patch changes."""
import glob
import hashlib
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
import rust_index as R  # noqa: E402

PATCHES = [os.path.join(ROOT, "integration", p) for p in ("lorikeet-hip.patch", "lorikeet-hip-shared-handle.patch")]
OUT = os.path.join(HERE, "reference_tree_facts.json")
# names the identifier test looks up to know that the index is the reference's own, though the patches do not use them
SENTINELS = {"compute_read_likelihoods"}
HUNK = re.compile(r"^@@ -(\d+)(?:,(\d+))? \+\d+(?:,\d+)? @@")


def window_hash(lines):
    return hashlib.sha256("".join(ln + "\n" for ln in lines).encode()).hexdigest()


def hunks(patch_text):
    """[(file, start, count)] of every hunk, in order (start is 1-based; count 0 means 'insert after line start')."""
    out, cur = [], None
    for ln in patch_text.splitlines():
        if ln.startswith("diff --git"):
            cur = ln.split(" b/")[1]
        m = HUNK.match(ln)
        if m:
            out.append((cur, int(m.group(1)), 1 if m.group(2) is None else int(m.group(2))))
    return out


def rust_index(reference, used):
    fns, items, fields, variants, impls = {}, set(), set(), set(), {}
    for f in glob.glob(os.path.join(reference, "src", "**", "*.rs"), recursive=True):
        t = R.strip(open(f).read())
        d = R.definitions(t)
        for k, v in d[0].items():
            fns.setdefault(k, set()).update(v)
        items |= d[1]
        fields |= d[2]
        variants |= d[3]
        for m in re.finditer(r"\bimpl\b\s*(?:<[^{]*?>\s*)?(?:[A-Za-z_][\w:]*(?:<[^{]*?>)?\s+for\s+)?([A-Za-z_]\w*)[^{;]*\{", t):
            end = R._match(t, m.end() - 1, "{", "}")
            for k, v in R.definitions(t[m.end():end - 1])[0].items():
                impls.setdefault(m.group(1), {}).setdefault(k, set()).update(v)
    return {"sizes": {"fns": len(fns), "items": len(items), "fields": len(fields), "variants": len(variants), "impls": len(impls)},
            "fns": {k: sorted(v) for k, v in sorted(fns.items()) if k in used},
            "items": sorted(items & used), "fields": sorted(fields & used), "variants": sorted(variants & used),
            "impls": {t: {k: sorted(v) for k, v in sorted(m.items()) if k in used} for t, m in sorted(impls.items()) if t in used}}


def main():
    reference = sys.argv[1]
    texts = [open(p).read() for p in PATCHES]
    added = "\n".join(ln[1:] for t in texts for ln in t.splitlines() if ln.startswith("+") and not ln.startswith("+++"))
    used = set(re.findall(r"[A-Za-z_]\w*", R.strip(added))) | SENTINELS
    base = {}
    for f, start, count in hunks(texts[0]):
        path = os.path.join(reference, f)
        if not os.path.exists(path):
            base[f] = {"exists": False}
            continue
        lines = open(path).read().split("\n")
        if lines and lines[-1] == "":
            lines.pop()
        e = base.setdefault(f, {"exists": True, "lines": len(lines), "hunks": {}})
        e["hunks"]["%d,%d" % (start, count)] = window_hash(lines[start - 1:start - 1 + count])
    json.dump({"rust_index": rust_index(reference, used), "patch_base": base}, open(OUT, "w"), indent=0, sort_keys=True)
    print(len(base), "files,", sum(len(e.get("hunks", {})) for e in base.values()), "hunks ->", OUT)


if __name__ == "__main__":
    main()
