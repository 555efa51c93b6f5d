"""The polynomial coefficients of wsmc_lgamma (include/wsmc_math.h), printed as C.

    python tools/gen_lgamma_coef.py

Three Chebyshev-node fits in 60-digit arithmetic (mpmath.chebyfit: near-minimax), each printed
lowest degree first with the fit's own maximal error:
  G  lgamma(2 + y) / y            y in [-1/2, 1/2]   (the pieces around the zeros at 1 and 2)
  H  lgamma(1 + x) / x            x in [0, 1/2]      (x < 1/2: lgamma(x) = x H(x) - log x)
  W  x (lgamma(x) - (x - 1/2)(log x - 1) - (log(2 pi) - 1) / 2),  as a polynomial in 1/x^2 on
     [0, 1/64]                                       (the Stirling correction for x >= 8)
"""
import mpmath as mp

mp.mp.dps = 60


def g(y):
    # below 1e-20 the two-term series (the quotient would lose the working precision)
    return mp.loggamma(2 + y) / y if abs(y) > 1e-20 else 1 - mp.euler + y * (mp.zeta(2) - 1) / 2


def h(x):
    return mp.loggamma(1 + x) / x if abs(x) > 1e-20 else -mp.euler + x * mp.zeta(2) / 2


W0 = (mp.log(2 * mp.pi) - 1) / 2


def w(z):
    if z == 0:
        return mp.mpf(1) / 12
    x = 1 / mp.sqrt(z)
    return x * (mp.loggamma(x) - (x - mp.mpf(1) / 2) * (mp.log(x) - 1) - W0)


def show(name, f, lo, hi, n):
    c, err = mp.chebyfit(f, [lo, hi], n, error=True)
    c = [float(v) for v in reversed(c)]   # lowest degree first, rounded to double
    print(f"/* {name}: degree {n - 1} on [{lo}, {hi}], fit error {mp.nstr(err, 3)} */")
    for k, v in enumerate(c):
        print(f"    {name}{k} = {v!r},")


if __name__ == "__main__":
    show("G", g, mp.mpf(-1) / 2, mp.mpf(1) / 2, 20)
    show("H", h, mp.mpf(0), mp.mpf(1) / 2, 17)
    show("W", w, mp.mpf(0), mp.mpf(1) / 64, 8)
    print("WSMC_LGAMMA_W0 =", repr(float(W0)))
