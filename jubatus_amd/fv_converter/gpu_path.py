"""GPU fv_converter fast path (host half).

Decides whether a converter config runs on the GPU and packs its rules
into the device rule tables.

* fast path (``fast_eligible``, csrc/hip/fv_hash.hip + scan.hip, one slot
  per (value, rule row)): no string filters, no binary or combination rules;
  every string rule is of built-in type ``str`` with global weight ``bin``;
  every num rule is ``num`` or ``log``; key matchers ``*``, prefix, suffix,
  exact. Num filters with a built-in method (``add``,
  ``linear_normalization``, ``gaussian_normalization``,
  ``sigmoid_normalization``) run there too: every chain of filters
  ``f1 < f2 < ...`` that can fire, followed by a num rule, is one more row of
  the num rule table (layout: csrc/hip/jb_fv.hpp), up to
  ``MAX_FILTER_CHAINS`` chains. For example ::

      "num_filter_types": {"z": {"method": "gaussian_normalization",
                                 "average": 170, "standard_deviation": 8}},
      "num_filter_rules": [{"key": "height", "type": "z", "suffix": "_z"}],
      "num_rules":        [{"key": "*", "type": "num"}]

  packs the base row (``*``, ``@num``) and the derived row of chain ``(0,)``
  with suffix ``_z@num``: two slots per num value;
* wide rule set (``wide_eligible``, csrc/hip/fv_wide.hip and the native host
  twin csrc/native/jb_hostfv_wide.hpp): adds the ``space`` / ``ngram``
  splitters, tf / log_tf with idf / bm25 global weights and add / mul
  combinations. Num filters run there under the same conditions and as the
  same derived rows (one packing helper, ``_pack_num_rows``); what differs is
  the feature order, which the combination pairs ``i < j`` depend on. The
  Python converter appends the derived values filter by filter, so a datum's
  num features come in blocks: the original values, then one block per chain
  in ``_filter_chains`` order, each block in datum order with the base rules
  innermost. With two ``*`` filters ``_0`` / ``_1``, values ``a``, ``b`` and
  the rule ``*`` that is ``a b a_0 b_0 a_1 b_1 a_0_1 b_0_1`` (``@num``). The
  kernels and the host twin walk the datum's num values once per block. A
  combination matcher sees a derived feature by its full name
  (``height_z@num``). The device converts at most 4096 base features per
  datum (``kWideMaxBase``) and derived features count: with 16 chains every
  num value is up to 17 features, so a datum reaches the limit 17 times
  sooner and then fails as before, ``TypeError("malformed datum (device wide
  converter)")``. The native servers keep running filters of wide configs
  through ``WideExt`` on the host.

``gpu_eligible`` is either; regex matchers, string filters, plug-in
("dynamic") filters, filter configs above the chain cap and plug-ins keep the
host converter.
"""
from __future__ import annotations

import math
import struct

import numpy as np

from .converter import DatumToFvConverter

_RULE = struct.Struct("<iiiiiifi")  # mirrors jb::GpuRule
_KIND = {"all": 0, "prefix": 1, "suffix": 2, "exact": 3}


# ---- num filters as derived num rows (csrc/hip/jb_fv.hpp, csrc/native/jb_hostfv.hpp)
# csrc/native/jb_fv_layout.hpp kMaxFilterChains. The device stages the rule blob
# in LDS up to 1024 bytes (fv_hash.hip kBlobCap); with many chains (seven and one
# rule: 0.6 KB, fifteen: 1.4 KB) the blob exceeds that and the kernel reads it from global
# memory instead: correct and tested, its cost not measured.
MAX_FILTER_CHAINS = 16
_DERIVED_ROW = 0x100            # kDerivedRow: value_kind bit of a filter-chain row
_STEP = struct.Struct("<iiiiiidd")   # mirrors jb::FilterStep
_METHOD = {"add": 0, "linear_normalization": 1, "gaussian_normalization": 2,
           "sigmoid_normalization": 3}


def _filter_steps(conv: DatumToFvConverter):
    """the num filter rules as (matcher kind, matcher bytes, suffix bytes,
    method, a, b, truncate), or None when one of them needs the host converter
    (a plug-in method, a regex key). The parameters are read as converter.py
    reads them."""
    types = conv.config.get("num_filter_types") or {}
    out = []
    for rule, (m, _, suffix) in zip(conv.config.get("num_filter_rules") or [], conv.num_filters):
        p = types.get(rule["type"]) or {}
        method = p.get("method")
        if method not in _METHOD or m.kind not in _KIND:
            return None
        a, b, trunc = 0.0, 0.0, 0
        if method == "add":
            a = float(p["value"])
        elif method == "linear_normalization":
            a, b = float(p["min"]), float(p["max"])
            trunc = int(str(p.get("truncate", "true")).lower() != "false")
        elif method == "gaussian_normalization":
            a, b = float(p["average"]), float(p["standard_deviation"])
        else:
            a, b = float(p["gain"]), float(p["bias"])
        out.append((_KIND[m.kind], m.arg.encode(), suffix.encode(), _METHOD[method], a, b, trunc))
    return out


def _bytes_match(kind: int, arg: bytes, key: bytes) -> bool:
    return (kind == 0 or (kind == 1 and key.startswith(arg)) or
            (kind == 2 and key.endswith(arg)) or (kind == 3 and key == arg))


def _filter_chains(steps):
    """every chain (f1 < f2 < ...) of filter indices that can fire, in the
    order converter.py _filtered appends the derived values, or None above
    MAX_FILTER_CHAINS. Pruned: once an exact matcher has fixed the original
    key, every later step is decided here; an exact matcher whose argument
    does not end with the suffixes appended so far never matches."""
    chains = [((), None, b"")]          # (indices, the key if known, suffixes so far)
    for f, (kind, arg, suffix, *_rest) in enumerate(steps):
        for idx, known, ext in list(chains):
            if known is not None:
                if not _bytes_match(kind, arg, known + ext):
                    continue
            elif kind == 3:
                if not arg.endswith(ext):
                    continue
                known = arg[:len(arg) - len(ext)]
            chains.append((idx + (f,), known, ext + suffix))
            if len(chains) - 1 > MAX_FILTER_CHAINS:
                return None
    return [c[0] for c in chains[1:]]


def _filters_ok(conv: DatumToFvConverter) -> bool:
    """the num filters (if any) run as derived num rows: built-in methods,
    non-regex keys, at most MAX_FILTER_CHAINS chains"""
    if not conv.num_filters:
        return True
    steps = _filter_steps(conv)
    return steps is not None and _filter_chains(steps) is not None


def _put(blob: bytearray, b: bytes) -> tuple[int, int]:
    off = len(blob)
    blob.extend(b)
    return off, len(b)


def _pack_num_rows(conv: DatumToFvConverter, blob: bytearray, is_log) -> tuple[list, int, int]:
    """The num rule table of both device paths (GpuRuleTable, WideRuleTable),
    appended to `blob`: the base rows (matcher and "@type" bytes, as before
    filters were served), then the filters' matcher bytes, the chain programmes
    (8-byte aligned) and one derived row per (chain, base row), chain-major,
    with the chain's suffixes + "@type" as its suffix. `is_log(rule)` tells a
    `log` row. -> (packed rows, base rows, chains)"""
    nrows, base = [], []
    for r in conv.num_rules:
        mo, ml = _put(blob, r.matcher.arg.encode())
        tail = f"@{r.type_name}".encode()
        so, sl = _put(blob, tail)
        vk = 1 if is_log(r) else 0
        base.append((_KIND[r.matcher.kind], mo, ml, tail, vk))
        nrows.append(_RULE.pack(_KIND[r.matcher.kind], mo, ml, so, sl, vk, 0.0, 0))
    chains = []
    if conv.num_filters:
        steps = _filter_steps(conv)
        chains = _filter_chains(steps)
        args = [_put(blob, st[1]) for st in steps]
        progs = []
        for chain in chains:
            blob.extend(b"\0" * (-len(blob) % 8))
            prog, ext = bytearray(), 0
            for f in chain:
                kind, _, suffix, method, a, b, trunc = steps[f]
                prog += _STEP.pack(kind, args[f][0], args[f][1], ext, method, trunc, a, b)
                ext += len(suffix)
            progs.append(_put(blob, struct.pack("<ii", len(chain), ext) + bytes(prog))[0])
        for chain, po in zip(chains, progs):
            ext = b"".join(steps[f][2] for f in chain)
            for kind, mo, ml, tail, vk in base:
                so, sl = _put(blob, ext + tail)
                nrows.append(_RULE.pack(kind, mo, ml, so, sl, vk | _DERIVED_ROW, 0.0, po))
    return nrows, len(base), len(chains)


def fast_eligible(conv: DatumToFvConverter) -> bool:
    """the fixed-slot fast path (fv_hash.hip / scan.hip): one slot per
    (value, rule row), constant string weights; num filters with a built-in
    method as derived num rows, up to MAX_FILTER_CHAINS chains"""
    if conv.string_filters or conv.binary_rules or conv.combination_rules:
        return False
    for r in conv.string_rules:
        if r.type_name != "str" or r.splitter is not None or r.gw != "bin":
            return False
        if r.matcher.kind not in _KIND:
            return False
    for r in conv.num_rules:
        if r.type_name not in ("num", "log") or r.matcher.kind not in _KIND:
            return False
    return _filters_ok(conv)


class GpuRuleTable:
    """Packed rule tables: (string rules, num rules, byte blob). The num
    rules are the base rows, then one derived row per (filter chain, base
    row), chain-major; the blob holds the matcher and suffix bytes of the
    base rows as before, then the filters' matcher bytes, the chain
    programmes (8-byte aligned) and the derived rows' suffixes."""

    def __init__(self, conv: DatumToFvConverter):
        if not fast_eligible(conv):
            raise ValueError("converter config is not eligible for the GPU fast path")
        blob = bytearray()
        srows = []
        for r in conv.string_rules:
            mo, ml = _put(blob, r.matcher.arg.encode())
            so, sl = _put(blob, r.suffix.encode())
            w = {"bin": 1.0, "tf": 1.0, "log_tf": math.log(2.0)}[r.sw]
            srows.append(_RULE.pack(_KIND[r.matcher.kind], mo, ml, so, sl, 0, w, 0))
        nrows, self.n_base, self.n_chains = _pack_num_rows(
            conv, blob, lambda r: r.type_name == "log")
        self.n_srules = len(srows)
        self.n_nrules = len(nrows)
        self.srules = np.frombuffer(b"".join(srows) or b"\0" * _RULE.size, dtype=np.uint8).copy()
        self.nrules = np.frombuffer(b"".join(nrows) or b"\0" * _RULE.size, dtype=np.uint8).copy()
        self.blob = np.frombuffer(bytes(blob) or b"\0", dtype=np.uint8).copy()
        self.H = conv.hash_max_size


# ------------------------------------------------------------- wide rule set
# string rule value_kind = splitter | sample_weight << 4 | global_weight << 8
# (csrc/native/jb_hostfv_wide.hpp, csrc/hip/fv_wide.hip); pad = ngram length
_SPLIT = {"str": 0, "ngram": 1, "space": 2}
_SW = {"bin": 0, "tf": 1, "log_tf": 2}
_GW = {"bin": 0, "idf": 1, "bm25": 2}
_COMB = {"add": 0, "mul": 1}


def wide_eligible(conv: DatumToFvConverter) -> bool:
    """configs the wide native / GPU converter reproduces exactly: str /
    space / ngram splitters, every sample and global weight, num / log num
    types, add / mul combinations; num filters where the fixed-slot path
    takes them (built-in method, non-regex key, up to MAX_FILTER_CHAINS
    chains); no string filters, plug-ins or regex matchers"""
    if conv.string_filters or conv.binary_rules or not _filters_ok(conv):
        return False
    for r in conv.string_rules:
        if r.split_kind not in _SPLIT or r.matcher.kind not in _KIND:
            return False
        if r.split_kind == "ngram" and r.split_n <= 0:
            return False
    for r in conv.num_rules:
        if r.kind not in ("num", "log") or r.matcher.kind not in _KIND:
            return False
    for ml, mr, tname, _ in conv.combination_rules:
        if conv.combination_methods.get(tname) not in _COMB:
            return False
        if ml.kind not in _KIND or mr.kind not in _KIND:
            return False
    return True


class WideRuleTable:
    """Packed wide rule tables: string rules, num rules (the base rows, then
    the derived rows of the filter chains, packed by the helper GpuRuleTable
    uses: ``n_base`` base rows, ``n_chains`` chains, ``n_nrules`` =
    ``n_base * (1 + n_chains)``), combination rules (two entries each: left
    matcher + "/type" suffix + op, right matcher)."""

    def __init__(self, conv: DatumToFvConverter):
        if not wide_eligible(conv):
            raise ValueError("converter config is not eligible for the wide native path")
        blob = bytearray()
        srows = []
        for r in conv.string_rules:
            mo, ml = _put(blob, r.matcher.arg.encode())
            so, sl = _put(blob, r.suffix.encode())
            vk = _SPLIT[r.split_kind] | _SW[r.sw] << 4 | _GW[r.gw] << 8
            srows.append(_RULE.pack(_KIND[r.matcher.kind], mo, ml, so, sl, vk, 0.0, r.split_n))
        nrows, self.n_base, self.n_chains = _pack_num_rows(conv, blob, lambda r: r.kind == "log")
        crows = []
        for ml_, mr_, tname, _ in conv.combination_rules:
            lo, ll = _put(blob, ml_.arg.encode())
            so, sl = _put(blob, f"/{tname}".encode())
            ro, rl = _put(blob, mr_.arg.encode())
            crows.append(_RULE.pack(_KIND[ml_.kind], lo, ll, so, sl,
                                    _COMB[conv.combination_methods[tname]], 0.0, 0))
            crows.append(_RULE.pack(_KIND[mr_.kind], ro, rl, 0, 0, 0, 0.0, 0))
        self.n_srules = len(srows)
        self.n_nrules = len(nrows)
        self.n_crules = len(crows) // 2
        self.srules = np.frombuffer(b"".join(srows) or b"\0" * _RULE.size, dtype=np.uint8).copy()
        self.nrules = np.frombuffer(b"".join(nrows) or b"\0" * _RULE.size, dtype=np.uint8).copy()
        self.crules = np.frombuffer(b"".join(crows) or b"\0" * _RULE.size, dtype=np.uint8).copy()
        self.blob = np.frombuffer(bytes(blob) or b"\0", dtype=np.uint8).copy()
        self.H = conv.hash_max_size
        self.global_weights = conv.uses_global_weight


def gpu_eligible(conv: DatumToFvConverter) -> bool:
    """the GPU converts this config: the fixed-slot fast path (built-in num
    filters included) or the wide rule-set kernels (csrc/hip/fv_wide.hip:
    ngram / space, tf / idf / bm25 with the DF table in HBM, combinations,
    built-in num filters)"""
    return fast_eligible(conv) or wide_eligible(conv)
