"""Host lint of the stream contract (include/deepgrp_hip.h: "all work is enqueued asynchronously on [`stream`] unless a function says
it synchronises"): no blocking copy, memset or device-wide / null-stream synchronisation in deepgrp_amd/csrc outside the function
bodies listed here with their reason, and no kernel launch whose stream argument is a literal 0.  tests/test_gpu_streams.py checks
the same contract on the device; this keeps a new violation from being written in the first place."""
import glob
import os
import re

from conftest import ROOT

CSRC = os.path.join(ROOT, "deepgrp_amd", "csrc")

BLOCKING = {
    "hipMemcpy(": re.compile(r"\bhipMemcpy\s*\("),
    "hipMemset(": re.compile(r"\bhipMemset\s*\("),
    "hipDeviceSynchronize": re.compile(r"\bhipDeviceSynchronize\b"),
    "hipStreamSynchronize(null)": re.compile(r"\bhipStreamSynchronize\s*\(\s*(0|NULL|nullptr)\s*\)"),
}

# (file, function, call) -> (occurrences, reason).  A count, not a licence: one more blocking call in a listed body fails too.
ALLOWED = {
    ("api.hip", "upload_raw", "hipMemcpy("): (1, "model create: the upload is documented synchronous and reads a host vector that dies on return"),
    ("api.hip", "upload_stream", "hipMemcpy("): (1, "model create, as above"),
    ("api.hip", "dgrp_model_create", "hipMemcpy("): (10, "model create, as above (packed fragments, tables, attention tensors)"),
    ("api.hip", "dgrp_model_create_lstm", "hipMemcpy("): (2, "model create, as above"),
    ("mss_kernels.hip", "dgrp_mss_segments_host", "hipMemcpy("): (2, "documented synchronous; it has no stream argument"),
    ("mss_kernels.hip", "dgrp_mss_segments_host", "hipDeviceSynchronize"): (1, "no stream argument: it waits for the dgrp_mss_labels call on whatever stream that ran"),
    ("mask_kernels.hip", "dgrp_fasta_mask_batch", "hipMemcpy("): (3, "error-message path only, after the stream was synchronised: fetches the offending row"),
    ("eval_kernels.hip", "eval_prepare", "hipMemcpy("): (1, "error-message path of the row check only, after the stream was synchronised"),
}


def _strip_comments(text):
    text = re.sub(r"/\*.*?\*/", lambda m: re.sub(r"[^\n]", " ", m.group(0)), text, flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


def _functions(lines):
    """line index -> name of the top-level function whose body holds it (bodies open with '{' and close with '}' in column 0)."""
    owner, name = {}, None
    for i, line in enumerate(lines):
        if line.startswith("{") and name is None:
            j = i - 1
            while j > 0 and (lines[j][:1] in (" ", "\t") or not lines[j].strip()):
                j -= 1
            m = re.search(r"(\w+)\s*\(", lines[j])
            name = m.group(1) if m else "?"
        if name is not None:
            owner[i] = name
        if line.startswith("}"):
            name = None
    return owner


def _sources():
    files = sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")) + glob.glob(os.path.join(CSRC, "*.inc")))
    assert len(files) > 15
    for path in files:
        with open(path, encoding="utf-8") as fh:
            yield os.path.basename(path), _strip_comments(fh.read())


def test_no_blocking_call_outside_the_allow_list():
    seen, problems = {}, []
    for fname, text in _sources():
        lines = text.split("\n")
        owner = _functions(lines)
        for i, line in enumerate(lines):
            for what, rx in BLOCKING.items():
                for _ in rx.finditer(line):
                    key = (fname, owner.get(i, "<file scope>"), what)
                    seen[key] = seen.get(key, 0) + 1
                    if key not in ALLOWED:
                        problems.append(f"{fname}:{i + 1}: {what} in {key[1]}: {line.strip()}")
    for key, n in seen.items():
        if key in ALLOWED and n > ALLOWED[key][0]:
            problems.append(f"{key[0]}: {key[1]} holds {n} x {key[2]}, the allow-list knows {ALLOWED[key][0]} ({ALLOWED[key][1]})")
    assert not problems, "blocking HIP calls outside the allow-list:\n" + "\n".join(problems)
    stale = [k for k in ALLOWED if k not in seen]
    assert not stale, f"allow-list entries that match nothing any more: {stale}"
    assert all(reason for _n, reason in ALLOWED.values())


def _call_args(text, start):
    """Top-level arguments of the call whose '(' is at text[start]."""
    depth, args, cur = 0, [], []
    for ch in text[start:]:
        if ch in "([{":
            depth += 1
            if depth == 1:
                continue
        elif ch in ")]}":
            depth -= 1
            if depth == 0:
                args.append("".join(cur).strip())
                return args
        if ch == "," and depth == 1:
            args.append("".join(cur).strip())
            cur = []
        else:
            cur.append(ch)
    raise AssertionError("unbalanced call")


def test_no_kernel_launch_on_a_literal_null_stream():
    launches, problems = 0, []
    for fname, text in _sources():
        for m in re.finditer(r"\bhipLaunchKernelGGL\s*\(", text):
            if re.match(r"#\s*define", text[text.rfind("\n", 0, m.start()) + 1:m.start()].strip() or ""):
                continue
            args = _call_args(text, m.end() - 1)
            launches += 1
            line = text.count("\n", 0, m.start()) + 1
            if len(args) < 5:
                problems.append(f"{fname}:{line}: hipLaunchKernelGGL with {len(args)} arguments")
            elif re.fullmatch(r"\(?\s*(\(\s*hipStream_t\s*\))?\s*(0|NULL|nullptr)\s*\)?", args[4]):
                problems.append(f"{fname}:{line}: kernel {args[0]} launched on the literal stream {args[4]}")
        for m in re.finditer(r"<<<[^>]*>>>", text):
            cfg = [a.strip() for a in m.group(0)[3:-3].split(",")]
            launches += 1
            if len(cfg) < 4 or cfg[3] in ("0", "NULL", "nullptr"):
                problems.append(f"{fname}:{text.count(chr(10), 0, m.start()) + 1}: triple-chevron launch without the caller's stream")
    assert launches > 80, f"only {launches} launches found: the scan is broken"
    assert not problems, "\n".join(problems)


def test_the_lint_sees_what_it_is_meant_to_see():
    """The scanners on a synthetic body: each forbidden form is reported, the stream-ordered forms are not."""
    bad = "static int f(hipStream_t s)\n{\n    hipMemcpy(a, b, 4, k);\n    hipMemset (a, 0, 4);\n    hipDeviceSynchronize();\n    hipStreamSynchronize( nullptr );\n}\n"
    good = "static int g(hipStream_t s)\n{\n    hipMemcpyAsync(a, b, 4, k, s);  // hipMemcpy(\n    hipMemsetAsync(a, 0, 4, s);\n    hipStreamSynchronize(s);\n}\n"
    lines = _strip_comments(bad + good).split("\n")
    owner = _functions(lines)
    hits = [(owner[i], what) for i, ln in enumerate(lines) for what, rx in BLOCKING.items() if rx.search(ln)]
    assert hits == [("f", "hipMemcpy("), ("f", "hipMemset("), ("f", "hipDeviceSynchronize"), ("f", "hipStreamSynchronize(null)")]
    call = "hipLaunchKernelGGL((k<1, 2>), dim3((n + 3) / 4), dim3(256), 0, 0, a, b);"
    assert _call_args(call, call.index("("))[4] == "0"
    call = "hipLaunchKernelGGL(k, dim3(f(a, b)), dim3(64), lds, stream, x[0], 0);"
    assert _call_args(call, call.index("("))[4] == "stream"
