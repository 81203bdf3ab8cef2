! Path-length moments of local-estimate radiances through the Fortran shell: specifyParameters(computeRadiancePathLengths = .true.) and
! reportResults(radiancePathLength =, radiancePathLengthSquared =) on a small cloud over a reflecting surface, irregular layers, two
! view directions.  Prints the two arrays, direction after direction and column after column, and every direction's domain mean path
! -- sum(path) / sum(intensity), summed in double precision -- (tests/test_gpu_radiance_path_lengths.py runs the same photons through
! the Python mirror), and what the shell answers when the arrays are asked for without having been computed, into an array of the
! wrong shape, or while another diagnostic tally is on.
program radiancePathTest
  use ErrorMessages
  use RandomNumbers
  use scatteringPhaseFunctions
  use opticalProperties
  use monteCarloIllumination
  use monteCarloRadiativeTransfer
  implicit none
  integer, parameter :: nx = 4, ny = 2, nz = 6, nDir = 2, nPhotons = 20000
  type(ErrorMessage)         :: status
  type(domain)               :: cloud
  type(integrator)           :: mc
  type(randomNumberSequence) :: randoms
  type(photonStream)         :: photons
  type(phaseFunction)        :: hg
  type(phaseFunctionTable)   :: table
  real    :: ext(nx, ny, nz), ssa(nx, ny, nz), path1(nx, ny, nDir), path2(nx, ny, nDir), inten(nx, ny, nDir), wrong(nx, ny, nDir + 1)
  integer :: idx(nx, ny, nz), i, j, k, d

  hg = new_PhaseFunction(0.85**(/ (i, i = 1, 64) /), status = status)
  table = new_PhaseFunctionTable((/ hg /), key = (/ 1. /), status = status)
  do k = 1, nz
    do j = 1, ny
      do i = 1, nx
        ext(i, j, k) = 0.0002
        if(k >= 3 .and. k <= 5) ext(i, j, k) = 0.004 * (1 + mod(i + j, 3))
      end do
    end do
  end do
  ssa = 0.95; idx = 1
  cloud = new_Domain((/ 0., 500., 1000., 1500., 2000. /), (/ 0., 500., 1000. /), (/ 0., 100., 250., 300., 500., 800., 1000. /), status)
  call addOpticalComponent(cloud, "cloud", ext, ssa, idx, table, status = status)
  mc = new_Integrator(cloud, status)
  if(stateIsFailure(status)) then
    print *, "new_Integrator failed"; stop 1
  end if
  call specifyParameters(mc, surfaceAlbedo = 0.3, minInverseTableSize = 10001, intensityMus = (/ 1., 0.6 /), intensityPhis = (/ 0., 100. /), &
                         computeIntensity = .true., useRussianRouletteForIntensity = .true., zetaMin = 0.3, status = status)
  if(stateIsFailure(status)) then
    print *, "specifyParameters failed: ", trim(failureText()); stop 1
  end if

  ! asked for before it is switched on
  randoms = new_RandomNumberSequence(seed = (/ 7, 3 /))
  photons = new_PhotonStream(0.5, 30., numberOfPhotons = nPhotons, randomNumbers = randoms, status = status)
  call computeRadiativeTransfer(mc, randoms, photons, status)
  call finalize_PhotonStream(photons)
  call initializeState(status)
  call reportResults(mc, status = status, radiancePathLength = path1)
  print '(a, l2, 1x, a)', "unavailable ", stateIsFailure(status), trim(failureText())
  call initializeState(status)

  call specifyParameters(mc, status = status, computeRadiancePathLengths = .true.)
  if(stateIsFailure(status)) then
    print *, "specifyParameters(computeRadiancePathLengths) failed"; stop 1
  end if
  ! the diagnostic tallies share their place: the others are refused while this one is on
  call initializeState(status)
  call specifyParameters(mc, status = status, computePathLengths = .true.)
  print '(a, l2, 1x, a)', "exclusive   ", stateIsFailure(status), trim(failureText())
  call initializeState(status)
  randoms = new_RandomNumberSequence(seed = (/ 7, 3 /))
  photons = new_PhotonStream(0.5, 30., numberOfPhotons = nPhotons, randomNumbers = randoms, status = status)
  call computeRadiativeTransfer(mc, randoms, photons, status)
  if(stateIsFailure(status)) then
    print *, "computeRadiativeTransfer failed: ", trim(failureText()); stop 1
  end if
  call initializeState(status)
  call reportResults(mc, status = status, radiancePathLengthSquared = wrong)
  print '(a, l2, 1x, a)', "wrongshape  ", stateIsFailure(status), trim(failureText())
  call initializeState(status)
  call reportResults(mc, intensity = inten, status = status, radiancePathLength = path1, radiancePathLengthSquared = path2)
  if(stateIsFailure(status)) then
    print *, "reportResults failed: ", trim(failureText()); stop 1
  end if
  do d = 1, nDir
    print '(a, i2, 8es16.8)', "intensity", d, ((inten(i, j, d), i = 1, nx), j = 1, ny)
    print '(a, i2, 8es16.8)', "radPath1 ", d, ((path1(i, j, d), i = 1, nx), j = 1, ny)
    print '(a, i2, 8es16.8)', "radPath2 ", d, ((path2(i, j, d), i = 1, nx), j = 1, ny)
    print '(a, i2, 2es20.12)', "meanPath ", d, sum(dble(path1(:, :, d))) / sum(dble(inten(:, :, d))), &
                                              sum(dble(path2(:, :, d))) / sum(dble(inten(:, :, d)))
  end do
  ! switched off again: the arrays are gone
  call specifyParameters(mc, status = status, computeRadiancePathLengths = .false.)
  call initializeState(status)
  call reportResults(mc, status = status, radiancePathLength = path1)
  print '(a, l2)', "offagain    ", stateIsFailure(status)
  call finalize_Integrator(mc)
  print '(a)', "radiancePathTest done"
contains
  ! the oldest message of the status object (the probes start from a fresh one)
  function failureText() result(text)
    character(len = 256) :: text
    call firstMessage(status)
    text = getCurrentMessage(status)
  end function failureText
end program radiancePathTest
