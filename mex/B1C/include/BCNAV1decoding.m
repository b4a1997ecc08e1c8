function [eph, firstSubFrame, TOW] = BCNAV1decoding(trackResults, channelNr, settings)
% Drop-in for B1C/include/BCNAV1decoding.m on the GPU: frame synchronisation on the
% pilot's secondary code, BCH(21,6) / BCH(51,8) of sub-frame 1 in either polarity,
% de-interleaving, CRC-24Q of sub-frames 2 and 3 and the ephemeris fields of every
% frame that passes, all through bds_mex('nav_decode', ...) -> bds_nav_decode of
% libbds_mi355x.so.  No LDPC decoding, as in the reference.
%
%   [eph, firstSubFrame, TOW] = BCNAV1decoding(trackResults, channelNr, settings)
%
% eph has the fields of eph_structure_init ([] where nothing was decoded);
% firstSubFrame and TOW are inf where no frame passed.  A CRC-valid frame whose PRN
% field is outside 1..63 is not entered (the reference returns from ephemeris() early
% there and then finds TOW empty).
r = trackResults(channelNr);
if settings.pilotTRKflag == 2
    sync = r.Pilot_I_P;   % wide-band tracking: the pilot is on I
else
    sync = r.Pilot_Q_P;   % narrow-band tracking: the pilot is on Q
end
out = bds_mex('nav_decode', 1, r.PRN, double(sync(:).'), double(r.I_P(:).'));
eph = rmfield(out.eph, {'SOW', 'IODC_MSB2', 'IODC_LSB8', 'n_entered', 'idValid'});
types = {[], 'GEO', 'IGSO', 'MEO'};
eph.SatType = types{out.eph.SatType + 1};
if out.eph.flag == 0, eph.flag = []; end
firstSubFrame = out.firstSubFrame;
TOW = out.TOW;
end
