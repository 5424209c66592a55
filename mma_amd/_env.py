"""The one way the package reads its MMA_* environment switches (README.md lists every name)."""
import os


def flag(name, default=True):
    """An on/off switch: "0" turns it off, any other value leaves it on.  A default-off switch (default=False) is on only for "1"."""
    v = os.environ.get(name)
    return default if v is None else (v != "0" if default else v == "1")


def integer(name, default):
    """An integer plan parameter."""
    return int(os.environ.get(name, default))
