function [navSolutions, eph] = postNavigation(trackResults, settings)
% Drop-in for BDS-3_B2a/postNavigation.m on the GPU: the decoding loop runs through
% bds_mex('nav_decode', ...) channel by channel, everything behind it -- readiness,
% the measurement grid, pseudoranges, satellite positions and clocks, the least-squares
% fix with its elevation mask, DOP and geodetic coordinates -- through
% bds_mex('post_navigation', ...) -> bds_post_navigation of libbds_mi355x.so.
%
%   [navSolutions, eph] = postNavigation(trackResults, settings)
%
% navSolutions has the reference's fields.  utmZone, E, N and U come from the reference's
% own findUtmZone / cart2utm, which must be on the path (they are not part of the library).
% Rules that are the library's own (include/bds_mi355x.h): the T_GDB1Cp term of satpos,
% a field the B2a ephemeris does not have, is 0; a ready channel with an empty SatType is
% dropped; absoluteSample must increase strictly on every ready channel.

% the record-length gate
if (settings.msToProcess < 24000)
    disp('postNavigation: the record is shorter than 24 s; no navigation solution.');
    navSolutions = [];
    eph          = [];
    return
end

nCh = settings.numberOfChannels;
subFrameStart = inf(1, nCh);
TOW           = inf(1, nCh);
types = {[], 'GEO', 'IGSO', 'MEO'};
status = repmat('-', 1, nCh);
PRN    = zeros(1, nCh);

activeChnList = find([trackResults.status] ~= '-');
n = numel(trackResults(activeChnList(1)).absoluteSample);
absoluteSample = zeros(n, nCh);
codeFreq       = zeros(n, nCh);
remCodePhase   = zeros(n, nCh);
for channelNr = activeChnList
    r = trackResults(channelNr);
    out = bds_mex('nav_decode', 2, 1, double(r.I_P(:).'), []);
    raw(channelNr) = out.eph; %#ok<AGROW>  (idle channels in between: every field [])
    subFrameStart(channelNr) = out.firstSubFrame;
    TOW(channelNr)           = out.TOW;
    % eph(PRN) as BCNAV2decoding returns it
    e = rmfield(out.eph, {'SOH', 'HOW', 'IODC', 'IODE', 'T_GDB2ap', 'ISC_B1Cd', 'T_GDB1Cp', ...
                          'PageID1', 'PageID3', 'SISMAI', 'TOW', 'flag', 'n_entered'});
    e.SatType = types{out.eph.SatType + 1};
    eph(r.PRN) = e; %#ok<AGROW>
    status(channelNr) = 'T';
    PRN(channelNr)    = r.PRN;
    absoluteSample(:, channelNr) = r.absoluteSample(:);
    codeFreq(:, channelNr)       = r.codeFreq(:);
    remCodePhase(:, channelNr)   = r.remCodePhase(:);
end
if numel(raw) < nCh, raw(nCh).PRN = []; end

out = bds_mex('post_navigation', settings, 2, status, PRN, absoluteSample, codeFreq, remCodePhase, raw, subFrameStart, TOW);
if out.n_meas == 0
    disp('postNavigation: fewer than 4 channels are ready, or no measurement epoch fits; no navigation solution.');
    navSolutions = [];
    return
end
navSolutions = rmfield(out, {'n_meas', 'ready'});

% UTM coordinates by the reference's own functions
for currMeasNr = 1:out.n_meas
    if isnan(navSolutions.X(currMeasNr))
        navSolutions.E(currMeasNr) = NaN;
        navSolutions.N(currMeasNr) = NaN;
        navSolutions.U(currMeasNr) = NaN;
    else
        navSolutions.utmZone = findUtmZone(navSolutions.latitude(currMeasNr), navSolutions.longitude(currMeasNr));
        [navSolutions.E(currMeasNr), navSolutions.N(currMeasNr), navSolutions.U(currMeasNr)] = ...
            cart2utm(navSolutions.X(currMeasNr), navSolutions.Y(currMeasNr), navSolutions.Z(currMeasNr), navSolutions.utmZone);
    end
end
end
