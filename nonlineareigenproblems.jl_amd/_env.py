"""Readers of the package's NEP_* environment switches (DESIGN.md section 6 lists every one).  Nothing is cached: a site
that wants a value once per process keeps it in a name of its own."""
import os


def env_str(name, default=None):
    """the value as it stands, `default` when unset"""
    return os.environ.get(name, default)


def env_int(name, default):
    v = os.environ.get(name)
    return default if v is None else int(v)


def env_float(name, default):
    v = os.environ.get(name)
    return default if v is None else float(v)


def env_flag(name):
    """set to anything but the empty string ("0" counts as set); switches that default to on are written
    env_str(name, "1") != "0" at their site"""
    return bool(os.environ.get(name))
