// roster.h -- the speaker roster (sdhip.h: sd_roster_*): a host object that hands out speaker ids which keep their meaning from one update of a stream
// to the next and from one recording to another.  Host only: no HIP header, no context, nothing launched.  roster.cpp holds the rule and the entries
// that need no context (sd_roster_open / _close / _load / _info / _speakers / _update, sd_relabel_turns_map); api.cpp and stream.hip hold the ones that
// read a context or a stream.  tools/sanitize/roster_main.cpp builds roster.cpp alone under AddressSanitizer + UBSan.
#ifndef SD_ROSTER_H
#define SD_ROSTER_H
#include <stddef.h>
#include <stdint.h>
#include "../../include/sdhip.h"

// P entries: centroid cen[p][d], the train rows n[p] it was estimated from, seen[p] = the index of the last update that gave p out (-1: loaded and never
// given out); updates = the update counter U; attached = the streams that hold this roster (sd_roster_close refuses while > 0)
struct sd_roster {
    int d;
    int64_t P, cap;
    double* cen;
    int64_t* n;
    int64_t* seen;
    int64_t updates;
    int64_t attached;
};

// every allocation of roster.cpp goes through this pointer (malloc unless a test program replaces it: a null return is an allocation that failed)
extern void* (*roster_alloc_hook)(size_t bytes);

// a call that updates several rosters and may still fail behind them (sd_stream_turns_many) takes a copy first and puts it back on failure
int roster_copy(const sd_roster* r, sd_roster** out);        // SD_OK or SD_ERR_NOMEM
void roster_swap_tables(sd_roster* a, sd_roster* b);         // exchanges entries and counter; `attached` stays
void roster_free(sd_roster* r);
#endif
