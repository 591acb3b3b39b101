"""The two message-passing builtins that cornac/models/lightgcn/lightgcn.py names, as plain records: `multi_update_all` of the
stand-in graph (dgl/__init__.py) reads their fields."""
from collections import namedtuple

UMulE = namedtuple("UMulE", "u e out")
Sum = namedtuple("Sum", "msg out")


def u_mul_e(u, e, out):
    """message = source node feature `u` times edge feature `e`"""
    return UMulE(u, e, out)


def sum(msg, out):   # noqa: A001  (the name the reference calls)
    """reduce = sum of the incoming messages `msg` into node feature `out`"""
    return Sum(msg, out)
