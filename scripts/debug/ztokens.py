"""Diagnostic: a zlib stream (RFC 1950/1951) as its LZ77 tokens, to locate the
first parse decision where two encoders of the same input differ.
tokens(stream) -> list of (position, length, distance) with length 0 for a
literal (distance = the byte), and the block boundaries (positions).
The decoder lives with the test inputs (tests/deflate_cases.py), where the
deflate tests use it to name the first differing token of a failing strip."""
from __future__ import annotations

import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "tests"))
from deflate_cases import first_divergence, tokens  # noqa: E402,F401
