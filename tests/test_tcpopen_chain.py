"""The passive open end to end on the CPU: an ACCEPT record of
gcl_tcp_rx_open_host installed as a connection takes the handshake ACK through
gcl_tcp_rx_states_host to ESTABLISHED, and its SYN|ACK goes through
gcl_tx_hdr_host and gcl_l4_csum_host FILL into a frame whose option words and
TCP checksum are right and whose other bytes nobody touched.  No GPU."""
import numpy as np

from caladan_amd import gclassify as g
from tests import tcpopencases as oc


def test_accept_record_installs_and_the_handshake_ack_opens_it():
    c = oc.chain_case()
    out, _ = oc.run_host(g, c)
    assert out["verdict"][:4].tolist() == [oc.ACCEPT, oc.ACCEPT, oc.CLOSED_RST, oc.RST]
    r = out["open"][0]
    conn = np.zeros(1, dtype=g.TCP_CONN_DTYPE)
    # what tcp_rx_listener left in the PCB: snd_wnd is not known before the first ACK (the window of a SYN is
    # taken unscaled by the caller); snd_wl1 = irs so that the ACK (seq = irs + 1) updates the window
    for f in ("snd_una", "snd_nxt", "rcv_nxt", "rcv_wnd", "snd_wscale"):
        conn[f] = r[f]
    conn["snd_wnd"], conn["snd_wl1"], conn["snd_wl2"], conn["rcv_mss"] = 65535, r["irs"], r["iss"], 1460
    state = np.array([r["state"]], dtype=np.uint8)
    assert int(state[0]) == g.TCP_STATE_SYN_RECEIVED
    ack = oc.frame(oc.TACK, seq=int(r["rcv_nxt"]), ack=int(r["snd_nxt"]), lip=int(r["lip"]), rip=int(r["rip"]),
                   lport=int(r["lport"]), rport=int(r["rport"]))
    h = oc.case([(ack, 0)])
    res = g.tcp_rx_states_host(h["frames"], h["pkt_len"], h["sock"], conn, offs=h["offs"], state=state)
    assert int(res["state_out"][0]) == g.TCP_STATE_ESTABLISHED
    assert int(res["out_ext"][0]["xflags"]) & g.TCPX_OPENED
    assert int(res["ev"][0]) & g.TCPS_STATE and not int(res["ev"][0]) & (g.TCPS_RST | g.TCPS_RST_ACK)


def test_synack_through_tx_hdr_and_fill():
    c = oc.chain_case()
    out, hdr, st = oc.host_chain(g, c)
    k = int(out["seg_totals"][1])
    assert k == 4 and out["seg_kind"][:4].tolist() == [oc.K_SYNACK, oc.K_SYNACK, oc.K_RST, oc.K_RST]
    assert hdr["status"][:k].tolist() == [g.TXH_OK] * k
    assert hdr["pkt_len"][:k].tolist() == [62, 54, 54, 54]
    t = oc.tx(out)
    fo = [int(x) for x in out["frame_off"][:k]]
    # bytes 54-61 of the first SYN|ACK are tcp_put_options' two words: NOP WSCALE 3 rcv_wscale, MSS 4 rcv_mss
    assert t[fo[0] + 54:fo[0] + 62].tolist() == [1, 3, 3, 5, 2, 4, 0x05, 0xB4]
    assert t[fo[0] + 46] >> 4 == 7 and t[fo[0] + 47] == 0x12 and t[fo[1] + 46] >> 4 == 5
    assert int.from_bytes(t[fo[0] + 38:fo[0] + 42].tobytes(), "big") == int(out["open"][0]["iss"])
    assert int.from_bytes(t[fo[0] + 42:fo[0] + 46].tobytes(), "big") == 7001
    assert int.from_bytes(t[fo[1] + 42:fo[1] + 46].tobytes(), "big") == 0          # irs 0xFFFFFFFF + 1
    assert int.from_bytes(t[fo[0] + 48:fo[0] + 50].tobytes(), "big") == (1 << 20) >> 5
    # the checksum gcl_l4_csum VERIFY accepts, over the header and the options
    ver = g.l4_csum_host(t, hdr["pkt_len"], mode=g.L4_VERIFY, offs=out["frame_off"], n=k)
    assert (ver[:k] & 0xF).tolist() == [g.L4_GOOD] * k
    # nothing outside the four frames, and in the slots nothing behind the frame's own bytes
    keep = np.ones(len(t), dtype=bool)
    for x, ln in zip(fo, hdr["pkt_len"][:k].tolist()):
        keep[x:x + ln] = False
    assert (t[keep] == oc.SENTINEL).all()
    assert (out["tx_all"][:64] == oc.SENTINEL).all() and (out["tx_all"][-64:] == oc.SENTINEL).all()
