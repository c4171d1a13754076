"""What the request keywords of the decode loops (``sampling=``, ``penalties=``, ``logprobs=``, ``stop=``, ``ban=``,
``guide=``, ``dry=``, ``watermark=``, ``cut=``) have in common: how an argument and the process-wide default become the object a loop runs with."""
from __future__ import annotations


def resolve_keyword(value, cls, name: str, env, tail: str, temperature, use_env: bool):
    """The ``cls`` a loop runs with under keyword ``name``: the argument (refused at temperature > 0, the reference's own
    T > 0 path, with ``name= tail``); else, where `use_env` and no temperature is given, the default ``env()``."""
    if value is None:
        return env() if use_env and not temperature else None
    if not isinstance(value, cls):
        raise TypeError(f"{name} must be a longspec_amd.{cls.__name__} or None, got {type(value).__name__}")
    if temperature is not None and temperature > 0:
        raise ValueError(f"{name}= {tail}")
    return value
