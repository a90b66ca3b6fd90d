"""Pure-Python statement of the prompt-lookup rules the verify-and-propose tail implements (amq_lookup.hip; include/amq_hip.h) -- the reference the
CPU and GPU tests compare with.  No torch, no GPU."""


def propose(history, D, ngram_max):
    """drafts for the next step: for g = ngram_max .. 1, the MOST RECENT earlier occurrence in ``history`` of its last g tokens that is followed by at
    least one token; the up to D tokens behind it, unfilled slots -1"""
    history = list(history)
    L = len(history)
    for g in range(min(ngram_max, L - 1), 0, -1):
        suffix = history[L - g:]
        for s in range(L - g - 1, -1, -1):          # s + g <= L - 1: history[s + g] exists
            if history[s:s + g] == suffix:
                cont = history[s + g:s + g + D]
                return cont + [-1] * (D - len(cont))
    return [-1] * D


def accept(drafts, argmaxes):
    """(n, emitted): drafts[i - 1] is the token row i ran with (-1 = none), argmaxes[j] the arg-max of row j; n = the largest value with
    drafts[i - 1] == argmaxes[i - 1] for all 1 <= i <= n; the step emits argmaxes[0 .. n]"""
    n = 0
    while n < len(drafts) and drafts[n] >= 0 and drafts[n] == argmaxes[n]:
        n += 1
    return n, list(argmaxes[:n + 1])


def propose_brute(history, D, ngram_max):
    """the same rule restated as a search over (length, end) pairs instead of the nested loops above"""
    history = list(history)
    L = len(history)
    best = None                                     # (g, e): longest suffix match first, then the latest continuation start e
    for e in range(1, L):                           # history[e] exists: at least one token follows the occurrence that ends in front of e
        g = 0
        while g < ngram_max and e - 1 - g >= 0 and history[e - 1 - g] == history[L - 1 - g]:
            g += 1
        if g and (best is None or (g, e) > best):
            best = (g, e)
    if best is None:
        return [-1] * D
    cont = history[best[1]:best[1] + D]
    return cont + [-1] * (D - len(cont))


def step(history, drafts, argmaxes, D, ngram_max, external=False):
    """one verify-and-propose step on the host: -> (n, new history, next drafts)"""
    n, emitted = accept(drafts, argmaxes)
    new = list(history) + emitted
    return n, new, ([-1] * D if external else propose(new, D, ngram_max))
