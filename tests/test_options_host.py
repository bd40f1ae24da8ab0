"""The scoped option setter behind ``Context.options`` against a dictionary standing in for the library (no GPU)."""

import pytest

from draco_amd.device import scoped_options


class Store:
    """name -> value with the library's manners: an unknown name is a ``ValueError``; every call is logged."""

    def __init__(self, **values):
        self.values = {k.encode(): v for k, v in values.items()}
        self.log = []

    def get(self, name):
        self.log.append(("get", name))
        if name not in self.values:
            raise ValueError(f"unknown option '{name.decode()}'")
        return self.values[name]

    def set(self, name, value):
        self.log.append(("set", name, value))
        if name not in self.values:
            raise ValueError(f"unknown option '{name.decode()}'")
        self.values[name] = value

    def sets(self):
        return [e[1:] for e in self.log if e[0] == "set"]


def test_previous_values_come_back_in_reverse_order():
    s = Store(a=3, b=1, c=0)  # a and b are not at their defaults
    with scoped_options(s.get, s.set, dict(a=2, b=0, c=7)):
        assert s.values == {b"a": 2, b"b": 0, b"c": 7}
    assert s.values == {b"a": 3, b"b": 1, b"c": 0}
    assert s.sets() == [(b"a", 2), (b"b", 0), (b"c", 7), (b"c", 0), (b"b", 1), (b"a", 3)]
    assert [e[1] for e in s.log if e[0] == "get"] == [b"a", b"b", b"c"]  # each read once, before its set


def test_values_come_back_after_an_exception_in_the_body():
    s = Store(a=3, b=1)
    with pytest.raises(KeyError, match="from the body"):
        with scoped_options(s.get, s.set, dict(a=2, b=5)):
            assert s.values == {b"a": 2, b"b": 5}
            raise KeyError("from the body")
    assert s.values == {b"a": 3, b"b": 1}
    assert s.sets()[2:] == [(b"b", 1), (b"a", 3)]


def test_a_failing_set_restores_what_was_set_before_it():
    s = Store(a=3, c=4)
    entered = False
    with pytest.raises(ValueError, match="unknown option 'nope'"):
        with scoped_options(s.get, s.set, dict(a=2, nope=1, c=9)):
            entered = True
    assert not entered
    assert s.values == {b"a": 3, b"c": 4}
    assert s.sets() == [(b"a", 2), (b"a", 3)]  # the third was never attempted, the second not set again on the way out
    assert all(e[1] != b"c" for e in s.log)

    class ReadOnly(Store):  # the read succeeds, the set itself fails
        def set(self, name, value):
            if name == b"b":
                self.log.append(("set", name, value))
                raise ValueError("b cannot be set")
            super().set(name, value)

    r = ReadOnly(a=3, b=1, c=4)
    with pytest.raises(ValueError, match="b cannot be set"):
        with scoped_options(r.get, r.set, dict(a=2, b=5, c=9)):
            raise AssertionError("not reached")
    assert r.values == {b"a": 3, b"b": 1, b"c": 4}
    assert r.sets() == [(b"a", 2), (b"b", 5), (b"a", 3)]


def test_str_and_bytes_names_are_the_same_option():
    s, t = Store(a=3, b=1), Store(a=3, b=1)
    with scoped_options(s.get, s.set, {"a": 2, "b": 0}):
        inside_s = dict(s.values)
    with scoped_options(t.get, t.set, {b"a": 2, b"b": 0}):
        inside_t = dict(t.values)
    assert inside_s == inside_t == {b"a": 2, b"b": 0}
    assert s.log == t.log and s.values == t.values == {b"a": 3, b"b": 1}


def test_no_values_is_a_no_op():
    s = Store(a=3)
    with scoped_options(s.get, s.set, {}):
        pass
    assert s.log == [] and s.values == {b"a": 3}
