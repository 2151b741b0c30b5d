"""CPU: the case table of the stream-contract tests (tests/stream_cases.py) against include/radtxfr_hip.h and the ctypes
binding. Every function that takes a stream has a case or a named reason for having none; may_sync and the host-array flag
of a case are what the header says, sentence by sentence and parameter by parameter."""
import ctypes as C
import re

import stream_cases as S
from radtxfr_amd import _lib


def _declarations():
    """{name: [parameter names]} of every function the header declares."""
    code = re.sub(r"/\*.*?\*/", " ", S.header_text(), flags=re.S)
    out = {}
    for m in re.finditer(r"\b(rtx_\w+)\s*\(([^;{}()]*)\)\s*;", code):
        out[m.group(1)] = [p.strip().split()[-1].lstrip("*") for p in m.group(2).split(",") if p.strip() and p.strip() != "void"]
    return out


def test_every_stream_entry_has_a_case_or_a_reason():
    entries = S.stream_entries()
    assert len(entries) == len(set(entries)) > 40
    decl = _declarations()
    assert set(decl) == set(_lib.PROTOTYPES), set(decl) ^ set(_lib.PROTOTYPES)  # the parse sees what the binding lists
    for name in entries:
        assert name in _lib.PROTOTYPES and _lib.PROTOTYPES[name][1][-1] is C.c_void_p, name
        assert len(_lib.PROTOTYPES[name][1]) == len(decl[name]), name
        assert (name in S.SPECS) != (name in S.EXCLUDED), "%s: %s" % (name, "in both" if name in S.SPECS else "neither a case nor an exclusion")
    # and nothing else is in either table; no other prototype ends in a parameter called stream
    assert set(S.SPECS) | set(S.EXCLUDED) == set(entries)
    assert all(S.EXCLUDED.values())
    others = [n for n, p in decl.items() if n not in entries and p and p[-1].startswith("stream")]
    assert not others, others


def test_may_sync_is_what_the_header_says():
    text = S.header_text()
    entries = set(S.stream_entries())
    covered = 0
    for phrase, kind, bound in S.HEADER_SYNC:
        assert "synchronis" in phrase and kind in ("convention", "setup", "cold", "always"), phrase
        assert text.count(phrase) == 1, "not (or not once) in the header: %r" % phrase
        covered += phrase.count("synchronis")
        assert set(bound) <= entries, (phrase, set(bound) - entries)
        assert bool(bound) == (kind in ("cold", "always")), phrase
    # every sentence of the header that speaks of synchronising is accounted for: a new one fails here until it is read
    assert covered == text.count("synchronis"), (covered, text.count("synchronis"))
    always = S.always_sync_entries()
    for name, sp in S.SPECS.items():
        assert sp.may_sync == (name in always), name
    assert {n for n in S.EXCLUDED if n in always} == {"rtx_xs_lut_get_rows"}
    assert "rtx_cubic_resample" in always and "rtx_cubic_resample_unchecked" not in always


def test_host_array_cases_are_the_entries_with_host_parameters():
    """A parameter whose name ends in _h is a host array (the header's convention); knot_start is the one the header marks
    HOST in words."""
    decl = _declarations()
    assert "knot_start[nB + 1]: HOST" in S.header_text()
    want = {n for n in S.SPECS if any(p.endswith("_h") or p == "knot_start" for p in decl[n])}
    assert S.HOST_ARRAY_ENTRIES == want, S.HOST_ARRAY_ENTRIES ^ want


def test_two_stream_entries_are_the_headers_per_stream_owners():
    """The entries the header says own a workspace, a flag or a per-call table per (device, stream)."""
    two = {n for n, sp in S.SPECS.items() if sp.two_streams}
    assert two == {"rtx_ils", "rtx_srf_apply", "rtx_srf_moments", "rtx_srf_radiance_vjp", "rtx_srf_radiance_jvp", "rtx_tud_vjp",
                   "rtx_tud_jvp", "rtx_xs_od", "rtx_cubic_resample"}
    text = S.header_text()
    for phrase in ("per (device, stream)", "Calls on one stream share", "one per stream that has used it"):
        assert phrase in text
    assert all(sp.workspace for sp in S.SPECS.values() if sp.two_streams)
