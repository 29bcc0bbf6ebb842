"""The pool of a ResultSaver's buffer sets on its own (cutie_amd/inference/utils/saver_buffers.py Pool): a new set while fewer than the limit
are alive, else the taker blocks for the next one given back; a returned set of another key is dropped and replaced without exceeding the
limit; a reset forgets everything.  And the keyed cache next to it."""
import threading

from cutie_amd.inference.utils.saver_buffers import KeyedCache, Pool


class _Set:
    def __init__(self, *key):
        self.made_for = key


def test_the_pool_rule():
    made = []

    def make(*key):
        made.append(key)
        return _Set(*key)
    pool = Pool(3, make)
    sets = [pool.take(24, 40) for _ in range(3)]
    assert made == [(24, 40)] * 3 and pool.alive == 3 and len({id(s) for s in sets}) == 3
    assert all(s.pool is pool and s.key == (24, 40) for s in sets)
    # the fourth take blocks until the writer gives a set back
    got, taking = [], threading.Event()

    def taker():
        taking.set()
        got.append(pool.take(24, 40))
    t = threading.Thread(target=taker, daemon=True)
    t.start()
    assert taking.wait(10)
    t.join(0.2)
    assert t.is_alive() and not got and len(made) == 3
    pool.put(sets[1])
    t.join(10)
    assert not t.is_alive() and got == [sets[1]] and len(made) == 3 and pool.alive == 3
    # a returned set with another key is dropped and replaced: never more than the limit alive
    pool.put(sets[0])
    other = pool.take(37, 61)
    assert other is not sets[0] and other.key == (37, 61) and made[-1] == (37, 61) and len(made) == 4 and pool.alive == 3
    # ... also when the taker had to block for it
    t = threading.Thread(target=lambda: got.append(pool.take(37, 61)), daemon=True)
    t.start()
    t.join(0.2)
    assert t.is_alive()
    pool.put(sets[2])
    t.join(10)
    assert not t.is_alive() and got[-1].key == (37, 61) and got[-1] is not sets[2] and len(made) == 5 and pool.alive == 3
    # a recycled set of the right key comes back as it is
    pool.put(other)
    assert pool.take(37, 61) is other and len(made) == 5
    # a reset forgets everything: the sets given back and the count
    pool.put(other)
    pool.reset()
    assert pool.alive == 0
    fresh = [pool.take(37, 61) for _ in range(3)]
    assert other not in fresh and len(made) == 8 and pool.alive == 3


def test_a_pool_of_keyless_sets():
    pool = Pool(2, _Set)
    a, b = pool.take(), pool.take()
    pool.put(a)
    assert pool.take() is a and b.key == () and pool.alive == 2


def test_the_keyed_cache():
    made = []

    def make(v):
        def f():
            made.append(v)
            return v
        return f
    latest = KeyedCache(latest=True)
    assert latest.get('png', (24, 40), make('a')) == 'a' and latest.get('png', (24, 40), make('x')) == 'a'
    assert latest.get('jpeg', (24, 40), make('b')) == 'b'                    # another name: another slot
    assert latest.get('png', (37, 61), make('c')) == 'c' and latest.get('png', (24, 40), make('d')) == 'd'     # one key per name
    assert latest.get('jpeg', (24, 40), make('y')) == 'b'
    every = KeyedCache(latest=False)
    assert every.get('lut', (0, 5, 3), make('e')) == 'e' and every.get('lut', (0, 5, 3, 7), make('f')) == 'f'
    assert every.get('lut', (0, 5, 3), make('z')) == 'e'                     # the objects came back: the table is still there
    assert made == ['a', 'b', 'c', 'd', 'e', 'f']
    latest.clear()
    assert latest.get('png', (24, 40), make('g')) == 'g'
