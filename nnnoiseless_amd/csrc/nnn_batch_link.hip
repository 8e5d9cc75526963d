// nnn_batch_link.hip -- channel-linked gains (include/nnn_batch.h "Channel link"): set / get.  The link itself is applied
// in the gains sinks of the RNN kernels (link_quad of nnn_rnn.hip: rnn_gain_out4 in k_rnn and k_rnn_wf, the output layer's sink in k_back)
// and nowhere else.  There is no device memory behind it: the setting travels in every launch's argument block (Buffers::link), so a set
// made between two calls is ordered with them by that alone, and plan_group picks k_back's linking instantiation from the same fields.
// Needs nnn_batch_core.hip (fail, struct nnn_batch, refuse_pending, report_fault).
#pragma once

// every argument block (the ones a later nnn_batch_set_taps re-derives included): 0 = off, +-channels = max / min
static void link_publish(nnn_batch *h)
{
    const int v = h->link_ch > 1 ? (h->link_mode == NNN_LINK_MIN ? -h->link_ch : h->link_ch) : 0;
    for (int set = 0; set < NSET; set++) h->b[set].link = v;
}

// Everything a set can check, before it changes anything.  first: the batch's first stream in its owner's numbering (a node's shard: a
// link group may not straddle two shards; a batch of its own: 0).
int nnn_batch_check_channel_link(const nnn_batch *h, int channels, int mode, int first)
{
    if (!h) return fail("null batch");
    if (channels != 1 && channels != 2 && channels != 4) return fail("channels is %d: a link group has 1 (off), 2 or 4 channels", channels);
    if (mode != NNN_LINK_OFF && mode != NNN_LINK_MAX && mode != NNN_LINK_MIN) return fail("link mode %d is none of NNN_LINK_OFF, NNN_LINK_MAX, NNN_LINK_MIN", mode);
    if (h->S % channels != 0) return fail("%d streams are no whole number of %d-channel link groups", h->S, channels);
    if (first % channels != 0) return fail("first stream %d is not a multiple of %d: a link group would lie in two batches", first, channels);
    if (int rc = refuse_pending(h, "nnn_batch_set_channel_link")) return rc;
    return report_fault(h);
}

extern "C" int nnn_batch_set_channel_link(nnn_batch *h, int channels, int mode)
{
    if (int rc = nnn_batch_check_channel_link(h, channels, mode, 0)) return rc;
    const bool on = channels > 1 && mode != NNN_LINK_OFF;
    h->link_ch = on ? channels : 1;
    h->link_mode = on ? mode : NNN_LINK_OFF;
    link_publish(h);
    return 0;
}

// what the next processing call runs under: (1, NNN_LINK_OFF) while off, however it was switched off
extern "C" int nnn_batch_get_channel_link(const nnn_batch *h, int *channels, int *mode)
{
    if (!h) return fail("null batch");
    if (channels) *channels = h->link_ch;
    if (mode) *mode = h->link_mode;
    return 0;
}

// nnn_batch_clone: the clone takes h's link
static void link_clone(nnn_batch *c, const nnn_batch *h)
{
    c->link_ch = h->link_ch;
    c->link_mode = h->link_mode;
    link_publish(c);
}
