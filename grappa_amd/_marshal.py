"""What every binding of the C ABI shares: the error a failed entry point raises and the checks of a flat tensor argument."""
from __future__ import annotations

from typing import Optional

import torch


class GrappaHipError(RuntimeError):
    pass


_ERR = {-1: "GRAPPA_ERR_ARG (unsupported shape / null pointer)", -2: "GRAPPA_ERR_LAUNCH", -3: "GRAPPA_ERR_WORKSPACE"}


def _chk(rc: int, what: str) -> None:
    if rc != 0:
        raise GrappaHipError(f"{what} failed: {_ERR.get(rc, rc)}")


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _flat(t: torch.Tensor, name: str, dev, dtype=torch.float32) -> None:
    if t.dtype != dtype or t.device != dev or not t.is_contiguous():
        raise ValueError(f"{name}: expected a contiguous {dtype} tensor on {dev}")
