"""The tail words of the serial scratch are named twice: the enum of
csrc/hip/jb_serial_layout.hpp (what the kernels write) and TAIL_WORDS in
ops/hip.py (what SerialScratch.last_batch reads). The two must agree."""
import os
import re

from jubatus_amd.ops import hip

HEADER = os.path.join(os.path.dirname(hip.__file__), "..", "csrc", "hip", "jb_serial_layout.hpp")


def _header_enum():
    text = open(HEADER).read()
    body = re.search(r"enum\s*:\s*int\s*\{(.*?)\};", text, re.S)
    assert body, "tail word enum not found"
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"\b(kTail\w+)\s*=\s*(\d+)", body.group(1))}


def test_tail_words_match_header():
    words = _header_enum()
    assert words["kTailWords"] == 32 and len(words) > 20, words
    for name, index in hip.TAIL_WORDS.items():
        assert words.get(name) == index, (name, index, words.get(name))
    assert set(words) == set(hip.TAIL_WORDS)
    assert sorted(set(words.values())) == sorted(set(hip.TAIL_WORDS.values()))


def test_stop_reasons_match_header():
    text = open(HEADER).read()
    stops = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"\bkStop(\w+)\s*=\s*(\d+)", text)}
    assert stops == {name: i for i, name in enumerate(hip.STOP_REASONS)}, stops
