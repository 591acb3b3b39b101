"""The three message-passing builtins that cornac/models/ngcf/ngcf.py names, as plain records: `multi_update_all` of the
stand-in graph (dgl/__init__.py) reads their fields."""
from collections import namedtuple

CopyU = namedtuple("CopyU", "field out")
CopyE = namedtuple("CopyE", "field out")
Sum = namedtuple("Sum", "msg out")


def copy_u(u, out):
    """message = the source node's feature `u`"""
    return CopyU(u, out)


def copy_e(e, out):
    """message = the edge's feature `e`"""
    return CopyE(e, out)


def sum(msg, out):   # noqa: A001  (the name the reference calls)
    """reduce = sum of the incoming messages `msg` into node feature `out`"""
    return Sum(msg, out)
